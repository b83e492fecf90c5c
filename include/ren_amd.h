/* ren_amd.h -- C ABI of the MI355X-native (gfx950) Robust e-NeRF volume-rendering path.
 *
 * One shared object (robust_e_nerf_amd/csrc/libren_amd.so, built by
 * `hipcc --offload-arch=gfx950 -shared -fPIC`), `extern "C"` only, POD arguments.
 *
 * Conventions:
 *  - every `*_d` / unnamed array pointer is a DEVICE pointer owned by the caller
 *    (PyTorch-ROCm allocations); pointers documented "host" are read on the host
 *    before the launch (small descriptors: aabb, level table, scalars);
 *  - the library never allocates, frees or synchronises; kernels are enqueued on the
 *    `stream` argument (a hipStream_t passed as void*, 0 = default stream) and outputs
 *    are valid in stream order;
 *  - return value: REN_OK (0) or a negative ren_status; nothing throws across the ABI;
 *  - no mutable global state: the library is re-entrant, one process per GPU.
 *
 * Each entry point cites the reference interface (file:line under the reference repo)
 * it replaces.  Third-party ops the reference imports (nerfacc 0.3.1, tinycudann,
 * roma 1.2.7) are cited through their reference call sites.
 */
#ifndef REN_AMD_H
#define REN_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ren_status {
    REN_OK = 0,
    REN_ERR_BAD_ARG = -1,      /* null pointer / negative size / bad enum            */
    REN_ERR_UNSUPPORTED = -2,  /* configuration outside what the kernels implement   */
    REN_ERR_LAUNCH = -3        /* hipGetLastError() != hipSuccess after the launch   */
} ren_status;

/* nerfacc.ContractionType (robust_e_nerf/models/robust_e_nerf.py:214-218) */
enum { REN_CT_AABB = 0, REN_CT_TANH = 1, REN_CT_SPHERE = 2 };

#define REN_MAX_LEVELS 16

/* Multi-resolution hash grid level table (tcnn HashGrid; robust_e_nerf/external/ngp.py:166-170,
 * configs/train/synthetic.yaml:62-69).  Host struct, passed by pointer, copied into the
 * kernel arguments.  n_features_per_level is fixed at 2. */
typedef struct ren_grid_desc {
    int32_t  n_levels;                 /* <= REN_MAX_LEVELS; fused MLP kernels need 16     */
    float    scale[REN_MAX_LEVELS];    /* exp2f(l*log2f(b))*N_min - 1                      */
    uint32_t res[REN_MAX_LEVELS];      /* ceilf(scale)+1                                   */
    uint32_t size[REN_MAX_LEVELS];     /* entries in the level                             */
    uint32_t offset[REN_MAX_LEVELS];   /* first entry of the level                         */
    uint32_t hashed[REN_MAX_LEVELS];   /* 1 = spatial hash, 0 = dense index                */
} ren_grid_desc;

/* Scene / field geometry shared by the field kernels.  Host struct. */
typedef struct ren_scene_desc {
    float   aabb[6];                   /* NGPradianceField.aabb (ngp.py:152)               */
    int32_t contraction_type;          /* REN_CT_*  (ngp.py:231-237)                       */
} ren_scene_desc;

/* Packed sample stream (nerfacc packed layout; external/utils.py:106-119):
 *   ray_indices[n] int32, t_starts[n], t_ends[n] float32, sorted by ray.
 * rays_o / rays_d are (n_rays,3) float32.  Sample position = o + d*(t0+t1)/2
 * (external/utils.py:68-72). */

/* ---- library info ------------------------------------------------------------------ */
int ren_abi_version(void);                       /* bumps when a signature changes      */
/* Verification / tuning knobs: process-wide, read by the launch functions, initialised once from the environment
 * variable of the same name (REN_HGB_NO_PAIRS, ...).  None changes results.
 *   REN_KNOB_HGB_NO_PAIRS      1: single-update records on the hashed levels of the binned scatter as well
 *   REN_KNOB_HGB_HALVE_REGIONS 1: halve the bin regions so the overflow path (global atomics) runs
 *   REN_KNOB_MARCH_SEQUENTIAL  1: sequential occupancy marcher instead of the speculative one; 2 / 4 / 8 / 16: that many speculative
 *                              lanes per ray whatever the ray count (default: by ray count, csrc/ren_sampling.hip)
 *   REN_KNOB_HG_VARIANT        atomic hash-grid backward: bit 0 XCD-affine level mapping, bit 1 lane-pair atomics (default 2);
 *                              forward: bit 3 one workgroup row per level for the leading dense levels as well, instead of
 *                              the one row that walks them all (the mapping before the fused dense row; same features)
 *   REN_KNOB_VFIELD_PLAIN      1: arch mlp, bf16 mode: the forward / backward kernels without the software-pipelined epilogue
 *   REN_KNOB_HGB_SUBREGION     binned scatter, which of a pair bin's 8 sub-regions a workgroup appends to: 1 (default) = the one
 *                              of the XCD it runs on, 0 = (workgroup index / 8) % 8, i.e. every sub-region written from all XCDs
 *                              (the A/B of the per-XCD layout: same code, same cursors, only the line sharing differs) */
enum { REN_KNOB_HGB_NO_PAIRS = 0, REN_KNOB_HGB_HALVE_REGIONS = 1, REN_KNOB_MARCH_SEQUENTIAL = 2, REN_KNOB_HG_VARIANT = 3,
       REN_KNOB_VFIELD_PLAIN = 4, REN_KNOB_HGB_SUBREGION = 5, REN_KNOB_COUNT = 6 };
/* `activations` argument of the ren_mlp_* / ren_vanilla_* entry points (ABI 24; until ABI 23 a process-wide knob): the
 * activation alternatives of the YAML (models/nerf.py:8-29), i.e. MODEL configuration, passed per call so that renderers
 * with different sets can launch from different host threads / streams of one process.  Code: bits 0-1 base hidden layers
 * (0 softplus beta 100, 1 relu), bits 2-3 density (0 shifted_trunc_exp, 1 softplus, 2 shifted_softplus), bits 4-5 head hidden
 * layers (0 | 1 as the base), bits 6-7 radiance (0 softplus, 1 sigmoid).  0 = every shipped config.  The exact-f32 kernels
 * (ren_mlp_fwd/bwd[_save/_saved/_bf16], ren_mlp_fwd/bwd_jvp, ren_mlp_fwd_jvp2) take every code, the arch-mlp output heads
 * (ren_vanilla_heads_*) its density / radiance kinds; the bf16-matrix-core kernels (ren_mlp_*_x) and the fused arch-mlp field
 * (ren_vanilla_fwd / _bwd) implement code 0 only and return REN_ERR_UNSUPPORTED otherwise. */
int ren_set_knob(int32_t knob, int32_t value);    /* REN_OK or REN_ERR_BAD_ARG */
int ren_get_knob(int32_t knob);
const char *ren_build_info(void);                /* "gfx950 ..."                        */

/* ---- pose interpolation + ray generation ------------------------------------------
 * Replaces LinearTrajectory.forward (robust_e_nerf/models/trajectories.py:30-91, with
 * utils/tensor_ops.py:83-180 and roma 1.2.7) and NeRF.pixel_params_to_ray
 * (robust_e_nerf/models/nerf.py:206-228).
 * ts[B] float64 ns; tab_ts[C] int64; tab_pos[C,3], tab_quat[C,4] (XYZW) float32.
 * Outputs (any may be NULL): pos[B,3], rot[B,9] row-major. */
int ren_trajectory_fwd(const double *ts, int64_t B, const int64_t *tab_ts, const float *tab_pos,
                       const float *tab_quat, int64_t C, float *pos, float *rot, void *stream);
/* Kinv[9] device, px[B,2], pos[B,3], rot[B,9] -> rays_o[B,3], rays_d[B,3] */
int ren_raygen_fwd(const float *Kinv, const float *px, const float *pos, const float *rot,
                   int64_t B, float *rays_o, float *rays_d, void *stream);
/* both in one launch: rays_o/rays_d[R,3] of the poses at ts[R] through pixels px[i % px_rows] (px[px_rows,2]; the start
 * and end renders of a training step share the events' pixels: R = 2B, px_rows = B).  Same arithmetic as the two calls. */
int ren_pose_rays_fwd(const double *ts, int64_t R, const float *px, int64_t px_rows, const float *Kinv,
                      const int64_t *tab_ts, const float *tab_pos, const float *tab_quat, int64_t C,
                      float *rays_o, float *rays_d, void *stream);

/* ---- sampling ---------------------------------------------------------------------
 * nerfacc.ray_marching as called at robust_e_nerf/external/utils.py:106-119. */
/* ray_aabb_intersect: aabb host[6]; miss => t_min=t_max=1e10; t_min clamped >= 0.
 * near/far: pass NaN for "None" (external/utils.py:112-113).                          */
int ren_ray_aabb_intersect(const float *rays_o, const float *rays_d, int64_t n_rays,
                           const float *aabb_host, float near_plane, float far_plane,
                           float *t_min, float *t_max, void *stream);
/* Two-pass marching.  mode 0: occupancy-grid marching (reference semantics), mode 1:
 * uniform comb of n_uniform intervals over [t_min,t_max) (fixed-S sampler).
 * jitter[n_rays] (may be NULL): mode 0 -> t_min += u*step (stratified);
 *                               mode 1 -> comb shifted by u*delta.
 * binary: uint8/bool grid (res[0]*res[1]*res[2]), x-major.  roi host[6], res host[3].
 * Pass 1 (t_starts==NULL): writes counts[n_rays].  Pass 2: offsets[n_rays] (int64,
 * exclusive cumsum of counts) given, writes ray_indices/t_starts/t_ends.
 * interval_cache (optional, mode 0): float[n_rays * cache_cap * 2].  Pass 1 keeps the first cache_cap
 * intervals of every ray in it; pass 2 (same cache, and counts given as well) copies them instead of marching
 * again and re-marches only the rays with more than cache_cap samples.  Same output either way.
 * mode | REN_MARCH_VERIFIED_DIV: the three divisions by the roi's extents per visited cell run as a multiply-add sequence
 * that ren_march_div_check() has shown to be bit-identical to the division for THIS roi (same output; -15 % on the pass). */
#define REN_MARCH_VERIFIED_DIV 0x100
int ren_ray_march(const float *rays_o, const float *rays_d, const float *t_min,
                  const float *t_max, const float *jitter, int64_t n_rays,
                  const float *roi_host, const int32_t *res_host, const uint8_t *binary,
                  int32_t contraction_type, float step_size, float cone_angle,
                  int32_t mode, int32_t n_uniform,
                  const int64_t *offsets, int32_t *counts,
                  int32_t *ray_indices, float *t_starts, float *t_ends, float *interval_cache,
                  int32_t cache_cap, void *stream);
/* The write pass of ren_ray_march (either mode) that stores every sample's unit-cube position beside the stream:
 * x_unit[3 i ..] = contraction of `scene` applied to o + d (t0 + t1) / 2, the floats ren_hashgrid_fwd forms from the
 * stream itself (same operations, same fused multiply-adds), so that the encoder can take x_unit instead and does not
 * redo the ray fetch and the contraction once per level.  12 bytes per sample more in a launch that exists. */
int ren_ray_march_unit(const float *rays_o, const float *rays_d, const float *t_min,
                       const float *t_max, const float *jitter, int64_t n_rays,
                       const float *roi_host, const int32_t *res_host, const uint8_t *binary,
                       int32_t contraction_type, float step_size, float cone_angle,
                       int32_t mode, int32_t n_uniform,
                       const int64_t *offsets, int32_t *counts,
                       int32_t *ray_indices, float *t_starts, float *t_ends, float *interval_cache,
                       int32_t cache_cap, const ren_scene_desc *scene, float *x_unit, void *stream);

/* Exhaustive check behind REN_MARCH_VERIFIED_DIV: for each of the three extents b = roi[3 + k] - roi[k] (host floats, 2^-60 < b <
 * 2^60) every float a with 2^-100 < |a| < 2^100 is divided both ways -- a / b and q0 = a y, q = fma(fma(-q0, b, a), y, q0) with
 * y = RN(1 / b) -- and mismatches[0] (device) receives the number of pairs that differ in any bit (~1e10 divisions, ~20 ms; once
 * per scene box).  REN_ERR_UNSUPPORTED for a box with a corner coordinate of 0 (or below 2^-60): position differences could then
 * fall below the checked range.  The flag is for finite rays with |position| < 2^100. */
int ren_march_div_check(const float *roi, int64_t *mismatches, void *stream);
/* exclusive cumsum of counts[n] (int32) -> offsets[n] (int64), total[1] (int64) */
/* out[n] = iid U[0, 1) floats (24 bits), Philox4x32-10 keyed by `seed` at stream position `offset` (e.g. the step number): the
 * per-ray jitter of stratified sampling without a framework RNG launch (models/nerf.py:209-215 draws it with torch.rand). */
int ren_uniform(uint64_t seed, uint64_t offset, int64_t n, float *out, void *stream);
int ren_exclusive_scan(const int32_t *counts, int64_t n, int64_t *offsets, int64_t *total,
                       int64_t *scratch1024 /* int64[1024] device scratch, may be NULL (slow path) */, void *stream);

/* ---- device-side sample counts (ABI 24) ------------------------------------------------------------
 * The reference reads the number of marched / visible samples back to the host in the middle of every render
 * (external/utils.py:106-119, models/nerf.py:279-286) because it sizes the next tensors.  Entry points with an `n_dev`
 * argument take instead: n = the CAPACITY of the per-sample arrays (it sizes the launch), n_dev = device address of the real
 * count (int64); kernels work on min(n, *n_dev) samples.  n_dev == NULL: n is the count, as before.
 * ren_count_guard: after ren_exclusive_scan left the total on the device, compare it with the capacity.  Fits: *n_out =
 * total.  Does not fit: every counts[r] = 0 (the per-ray kernels write nothing: an empty render), *n_out = 0;
 * counts_also (may be NULL) is cleared with it -- the guard after the visibility pass clears the MARCHED counts as well,
 * which is what ren_compact_samples / ren_compact_features walk.
 * stats (may be NULL): stats[0] = the total as found, stats[1] = 1 if it did not fit, else 0.  The host reads `stats`
 * after it has enqueued the rest of the step -- a wait for the sampling kernels only -- and repeats an overflowed step
 * with larger arrays before the optimiser runs (engine.py: RenderCfg.device_counts).  ren_frag_zero_tail: zero the lanes beyond the count in the last 32-sample block of
 * a fragment-layout feature array (what the host-count path does before ren_compact_features). */
int ren_count_guard(int32_t *counts, int32_t *counts_also, int64_t n_rays, const int64_t *total, int64_t capacity,
                    int64_t *n_out, int64_t *stats, void *stream);
/* ren_exclusive_scan followed by ren_count_guard; ONE launch (one workgroup) for up to 65 536 rays */
int ren_scan_guard(int32_t *counts, int32_t *counts_also, int64_t n_rays, int64_t *offsets, int64_t *total, int64_t capacity,
                   int64_t *n_out, int64_t *stats, int64_t *scratch1024, void *stream);
int ren_frag_zero_tail(float *feat, int64_t capacity, const int64_t *n_dev, void *stream);

/* nerfacc.render_visibility inside ray_marching (sigma_fn branch): per ray
 * T = excl. cumprod(1-alpha); keep = T >= early_stop_eps (& alpha >= alpha_thre if >0).
 * Writes keep[n] (uint8) and kept_counts[n_rays]. */
int ren_visibility(const int64_t *offsets, const int32_t *counts, int64_t n_rays,
                   const float *sigmas, const float *t_starts, const float *t_ends,
                   float early_stop_eps, float alpha_thre, uint8_t *keep, int32_t *kept_counts,
                   void *stream);
/* stream compaction of the packed sample arrays by keep[] using new_offsets (exclusive
 * cumsum of kept_counts) */
int ren_compact_samples(const int64_t *offsets, const int32_t *counts, const int64_t *new_offsets,
                        int64_t n_rays, const uint8_t *keep, const float *t_starts,
                        const float *t_ends, int32_t *out_ray_indices, float *out_t_starts,
                        float *out_t_ends, void *stream);
/* ... which moves the kept samples' unit positions (ren_ray_march_unit) with them: x_unit[3 n] -> out_x_unit[3 n_kept] */
int ren_compact_samples_unit(const int64_t *offsets, const int32_t *counts, const int64_t *new_offsets,
                             int64_t n_rays, const uint8_t *keep, const float *t_starts,
                             const float *t_ends, const float *x_unit, int32_t *out_ray_indices, float *out_t_starts,
                             float *out_t_ends, float *out_x_unit, void *stream);
/* Fragment-layout features (32 floats per sample, see ren_hashgrid_fwd layout 1) of the kept samples, moved to
 * their compacted positions (same offsets/counts/new_offsets/keep as ren_compact_samples).  feat_out must hold
 * ceil(n_kept/32) blocks; the caller zeroes its last block (padding lanes). */
int ren_compact_features(const int64_t *offsets, const int32_t *counts, const int64_t *new_offsets, int64_t n_rays,
                         const uint8_t *keep, const float *feat_in, float *feat_out, void *stream);
/* (offsets, counts) from sorted ray_indices[n] (nerfacc unpack_info inverse) */
int ren_pack_info(const int32_t *ray_indices, int64_t n, int64_t n_rays, int64_t *offsets,
                  int32_t *counts, void *stream);

/* ---- multi-resolution hash grid ------------------------------------------------------
 * tcnn.Encoding HashGrid/Linear (robust_e_nerf/external/ngp.py:166-170,240).
 * Input either x_unit[n,3] (unit-cube positions; seam API) or, when x_unit==NULL, the
 * packed sample stream (positions formed and contracted in-kernel, ngp.py:231-237).
 * layout 0: feat[n, 2L] row-major (tcnn output);  layout 1: MFMA fragment order
 *   feat[((i>>5)*16 + l)*64 + f*32 + (i&31)]  (i sample, l level, f feature), n padded to 32. */
int ren_hashgrid_fwd(const ren_grid_desc *grid, const float *table, const float *x_unit,
                     const ren_scene_desc *scene, const float *rays_o, const float *rays_d,
                     const int32_t *ray_indices, const float *t_starts, const float *t_ends,
                     int64_t n, int32_t layout, float *feat, const int64_t *n_dev, void *stream);
/* x_unit[n,3] of a packed sample stream, as ren_hashgrid_fwd forms it from the stream: for streams whose writer did not
 * store it (one streaming launch), and what the sampler's own x_unit is held to */
int ren_unit_positions(const ren_scene_desc *scene, const float *rays_o, const float *rays_d,
                       const int32_t *ray_indices, const float *t_starts, const float *t_ends, int64_t n,
                       float *x_unit, const int64_t *n_dev, void *stream);
/* d(table) += scatter of dfeat (same layouts); atomics, non-deterministic order */
int ren_hashgrid_bwd(const ren_grid_desc *grid, float *grad_table, const float *x_unit,
                     const ren_scene_desc *scene, const float *rays_o, const float *rays_d,
                     const int32_t *ray_indices, const float *t_starts, const float *t_ends,
                     int64_t n, int32_t layout, const float *dfeat, void *stream);
/* Reverse-mode gradient w.r.t. the POSITION (tcnn's grid backward-input; csrc/ren_normals.hip):
 *   dx[i, :] = sum_l sum_f dfeat[i, l, f] * d feat[i, l, f] / d x[i, :]        dx[n, 3] float32, every row written
 * Positions and dfeat layouts as ren_hashgrid_fwd.  With x_unit the gradient is w.r.t. the unit-cube position (scene is
 * not read); from the sample stream it is the WORLD-space gradient at the sample midpoint: the unit-cube gradient times
 * the transposed Jacobian of the contraction (aabb, sphere, tanh).  The interpolation weights are piecewise linear, so the
 * gradient is the one of the cell ren_hashgrid_fwd reads for that point (it jumps at cell faces).  One launch, 128 corner
 * reads per sample, no atomics, reads the table only; deterministic. */
int ren_hashgrid_bwd_input(const ren_grid_desc *grid, const float *table, const float *x_unit,
                           const ren_scene_desc *scene, const float *rays_o, const float *rays_d,
                           const int32_t *ray_indices, const float *t_starts, const float *t_ends,
                           int64_t n, int32_t layout, const float *dfeat, float *dx, void *stream);

/* Same result as ren_hashgrid_bwd (grad_table += scatter of dfeat) but WITHOUT per-update global
 * atomics: the updates are counting-sorted by 16 384-entry table bin into `workspace` (HBM) and
 * each bin is accumulated in LDS, then added to the table with plain coalesced read-modify-writes
 * (see csrc/ren_hashgrid_binned.hip).  ~5x faster than the atomic scatter on MI355X, where global
 * atomics execute at the memory side.  workspace: ren_hashgrid_bwd_binned_workspace_bytes(n)
 * bytes of device scratch (1 280 B per sample + 64 KiB).  Needs level sizes <= 2^19. */
int64_t ren_hashgrid_bwd_binned_workspace_bytes(int64_t n);
int ren_hashgrid_bwd_binned(const ren_grid_desc *grid, float *grad_table, const float *x_unit,
                            const ren_scene_desc *scene, const float *rays_o, const float *rays_d,
                            const int32_t *ray_indices, const float *t_starts, const float *t_ends,
                            int64_t n, int32_t layout, const float *dfeat, void *workspace,
                            const int64_t *n_dev, void *stream);

/* ---- fused NGP MLPs --------------------------------------------------------------------
 * NGPradianceField.query_density / _query_rgb / forward (robust_e_nerf/external/ngp.py:230-280)
 * with MLP.forward (external/mlp.py:99-113), SHEncoder degree 4 (external/sh_encoder.py:28-93),
 * Softplus(beta=100) hidden, shifted_trunc_exp density, Softplus(beta=1) radiance
 * (models/nerf.py:17-29; configs/train/synthetic.yaml:72-84).
 * mlp_params: one device array of float32 in torch nn.Linear layout, concatenated:
 *   base.w0[64,32] base.b0[64] base.wo[16,64] base.bo[16]
 *   head.w0[64,31] head.b0[64] head.w1[64,64] head.b1[64] head.wo[C,64] head.bo[C]
 * feat: fragment layout (layout 1 above).  Per-sample geometry (selector ngp.py:238, view
 * direction) comes either from x_world[n,3] (+ dirs[n,3], may be NULL when density_only) -- the
 * field(x, dirs) seam -- or, when x_world==NULL, from the packed sample stream.
 * density_only!=0: only sigma is produced (sigma_fn pre-pass, external/utils.py:68-81;
 * occ_eval_fn, models/nerf.py:197-198).
 * base_out (may be NULL): raw base-MLP outputs, fragment layout [((i>>5)*8+g)*64+lane]
 * (ceil(n/32)*512 floats), saved for the backward pass. */
int ren_mlp_fwd(const float *mlp_params, int32_t radiance_dim, int32_t activations, const float *feat,
                const ren_scene_desc *scene, const float *x_world, const float *dirs,
                const float *rays_o, const float *rays_d, const int32_t *ray_indices,
                const float *t_starts, const float *t_ends, int64_t n, int32_t density_only,
                float *rgb, float *sigma, float *base_out, void *stream);
/* floats of device scratch ren_mlp_bwd needs for the per-wave weight-gradient slabs */
int64_t ren_mlp_bwd_workspace_floats(int32_t radiance_dim);
/* backward of ren_mlp_fwd: d_rgb[n,C], d_sigma[n] -> dfeat (fragment layout, ceil(n/32)*1024
 * floats) and grad_mlp_params (+=, same concatenated layout).  rgb = forward output;
 * d_base: scratch of ceil(n/32)*512 floats (gradient w.r.t. base_out, fragment layout);
 * workspace: ren_mlp_bwd_workspace_floats() floats.  Deterministic (no atomics). */
int ren_mlp_bwd(const float *mlp_params, int32_t radiance_dim, int32_t activations, const float *feat,
                const float *base_out, const ren_scene_desc *scene,
                const float *x_world, const float *dirs,
                const float *rays_o, const float *rays_d, const int32_t *ray_indices,
                const float *t_starts, const float *t_ends, int64_t n,
                const float *rgb, const float *d_rgb, const float *d_sigma,
                float *d_base, float *dfeat, float *grad_mlp_params, float *workspace, void *stream);

/* ---- volume rendering (packed) ----------------------------------------------------------
 * rendering() (robust_e_nerf/external/vol_rendering.py:16-128): nerfacc
 * render_weight_from_density + 3x accumulate_along_rays + background compose.
 * Outputs colors[n_rays,C], opacities[n_rays], depths[n_rays] (un-normalised, :111-126);
 * weights[n] and trans[n] (may be NULL) are saved for the backward pass / seam API.
 * bkgd[C] device (NULL = no background). */
int ren_composite_fwd(const int64_t *offsets, const int32_t *counts, int64_t n_rays,
                      const float *t_starts, const float *t_ends, const float *sigmas,
                      const float *rgbs, int32_t C, const float *bkgd,
                      float *colors, float *opacities, float *depths,
                      float *weights, float *trans, void *stream);
/* backward: g_colors[n_rays,C], g_opac[n_rays] (NULL=0), g_depth[n_rays] (NULL=0) and/or
 * g_weights[n] (NULL=0: per-sample upstream gradient of the weights themselves, i.e. the backward of
 * nerfacc.render_weight_from_density used on its own; then rgbs/g_colors/d_rgbs may be NULL)
 * -> d_sigmas[n], d_rgbs[n,C], d_bkgd_per_ray[n_rays,C] (NULL ok).
 * ren_composite_fwd with rgbs==NULL computes weights/trans/opacities/depths only. */
int ren_composite_bwd(const int64_t *offsets, const int32_t *counts, int64_t n_rays,
                      const float *t_starts, const float *t_ends, const float *sigmas,
                      const float *rgbs, int32_t C, const float *bkgd,
                      const float *weights, const float *trans, const float *opacities,
                      const float *g_colors, const float *g_opac, const float *g_depth,
                      const float *g_weights,
                      float *d_sigmas, float *d_rgbs, float *d_bkgd_per_ray, void *stream);

/* ---- event loss ------------------------------------------------------------------------------
 * ContrastThreshold.forward (models/event_generation_params.py:72-84), Loss.log_intensity_diff
 * (loss_metric/loss.py:32-74) and the 1/C^k normalisation + weighting of
 * RobustENeRF.training_step (models/robust_e_nerf.py:432-443,470-486), fused with its own
 * backward.  Inputs per event i: intensity_start/end[B] (render + min_modeled_intensity,
 * :867), target[B] (= ts_diff * ev_log_diff/(end-start), float32), valid[B] (uint8, NULL =
 * all valid).  err_fn: 0 l1, 1 mse, 2 mape.
 * fwd: loss_sum[2] (device) = {sum of errors over valid events, number of valid events}; the
 *      mean loss is loss_sum[0]/loss_sum[1] (an empty mask gives 0/0 = NaN like the reference).
 * bwd: g_start[B], g_end[B] = d(scale * mean error)/d(intensity); reads the count from
 *      loss_sum[1] on the device (no host sync); scale = param weight * loss weight. */
int ren_event_loss_fwd(const float *intensity_start, const float *intensity_end, const float *target,
                       const uint8_t *valid, int64_t B, int32_t err_fn, float *loss_sum, void *stream);
int ren_event_loss_bwd(const float *intensity_start, const float *intensity_end, const float *target,
                       const uint8_t *valid, int64_t B, int32_t err_fn, float scale,
                       const float *loss_sum, float *g_start, float *g_end, void *stream);

/* The same loss straight from the render outputs of the batched start / end pass (colors[2B, C], opacities[2B]; rows
 * [0, B) = start render): the intensity epilogue of RobustENeRF.render_pixels (models/robust_e_nerf.py:865-871: +
 * min_modeled_intensity, is_valid = opacity > 0 of either render when use_validity), `bayering` (:887-890: channel_idx[B]
 * uint8 or NULL), the log difference (:432-435) and the masked mean in ONE forward and ONE backward launch.
 * bwd writes g_colors[2B, C] (zeros in the channels an event does not see), and optionally intensity[2B], pred[B] (=
 * log I_end - log I_start), valid[B] and loss[1] = scale * loss_sum[0] / loss_sum[1] -- all on the device. */
int ren_event_diff_loss_fwd(const float *colors, const float *opacities, const uint8_t *channel_idx, int32_t C,
                            float min_intensity, const float *target, int32_t use_validity, int64_t B, int32_t err_fn,
                            float *loss_sum, void *stream);
int ren_event_diff_loss_bwd(const float *colors, const float *opacities, const uint8_t *channel_idx, int32_t C,
                            float min_intensity, const float *target, int32_t use_validity, int64_t B, int32_t err_fn,
                            float scale, const double *scale_dev, const float *loss_sum, float *g_colors, float *intensity,
                            float *pred, uint8_t *valid, float *loss, void *stream);
/* scale_dev (may be NULL): a device double that multiplies `scale` -- the 1/C^k param weight of a TRAINABLE mean contrast
 * threshold (event_params[4] = 1/C, [5] = 1/C^2 of ren_event_params_refresh), so that no kernel argument waits for a host
 * read of a parameter (robust_e_nerf.py:470-486). */

/* ---- event batch glue ---------------------------------------------------------------------------
 * ren_event_prepare: ContrastThreshold.forward and RefractoryPeriod.forward
 * (models/event_generation_params.py:72-84,196-203), the supervision timestamps of
 * RobustENeRF.training_step (models/robust_e_nerf.py:319-357) and both loss targets
 * (loss_metric/loss.py:39-42,63-66) for B events in one launch:
 *   ev = num_pos C_p - num_neg C_n (float32);  start = start_ts + tau (float64);
 *   ts_diff = (end - start) u_ts_diff;  ts_start = lerp(start, max(end - ts_diff, start), u_diff_start);
 *   ts_end = min(ts_start + ts_diff, end);  target_diff = float(ts_diff ev / (end - start));
 *   ts_grad = lerp(ts_start, ts_end, u_grad), target_grad = float(ev / (end - start))   [optional, NULL to skip];
 *   dts_* = d ts_* / d tau  [optional: only when the refractory period is trained].
 * ren_event_param_grad: d(loss term)/d(raw C_p/C_n ratio) and the direct d(loss term)/d(tau) through the loss
 * target with the rendered prediction held fixed -- the closed form of what the reference obtains by autograd
 * through event_generation_params.py:51-84 and loss.py:32-74 with the scaling of robust_e_nerf.py:470-486.
 * kind 0: pred = log I_end - log I_start against target_diff; kind 1: pred = d log I / dt against target_grad.
 * param_weight_power k: the 1/C^k normalisation (0: none).  Accumulates (+=) into ct_grad[1] (float32) and
 * tau_grad[1] (float64) on the device; either may be NULL. */
int ren_event_prepare(const int64_t *start_ts, const int64_t *end_ts, const int64_t *num_pos, const int64_t *num_neg,
                      const double *u_ts_diff, const double *u_diff_start, const double *u_grad, int64_t B, float c_p,
                      float c_n, double tau, double *ts_start, double *ts_end, float *target_diff, double *ts_grad,
                      float *target_grad, double *dts_start, double *dts_end, double *dts_grad, const double *event_params,
                      void *stream);
int ren_event_param_grad(int32_t kind, int32_t err_fn, int32_t param_weight_power, const float *pred,
                         const uint8_t *valid, const int64_t *start_ts, const int64_t *end_ts, const int64_t *num_pos,
                         const int64_t *num_neg, const double *u_ts_diff, int64_t B, float c_p, float c_n,
                         float raw_ratio, double tau, float weight, float *ct_grad, double *tau_grad,
                         const double *event_params, void *stream);
/* event_params (may be NULL: the scalar arguments count): device double[8] written by ren_event_params_refresh --
 * [0] C_p, [1] C_n, [2] raw ratio, [3] tau, [4] 1 / mean C, [5] 1 / (mean C)^2, [6] raw tau (clamped).  The kernels then take
 * C_p, C_n, raw and tau from there: with a trainable ratio / refractory period the step reads no parameter on the host.
 * ren_event_params_refresh: C_p = softplus(raw ratio) C_n (float32, event_generation_params.py:51-70); the raw refractory
 * period clamped to +-logit(1e-4) tau_max IN PLACE and tau = tau_max sigmoid(raw / tau_max) in float64 (:170-185,
 * modules.py:58-74).  ren_tau_adam_step: torch.optim.Adam (no weight decay) on that float64 scalar from d loss / d tau
 * (x d tau / d raw), state = {exp_avg, exp_avg_sq} on the device, `step` 1-based; clears tau_grad (robust_e_nerf.py:804-807). */
int ren_event_params_refresh(const float *ct_raw, float c_n, double *tau_raw, double tau_max, double *event_params,
                             void *stream);
int ren_tau_adam_step(double *tau_raw, double *tau_grad, double *state, double tau_max, double lr, double beta1, double beta2,
                      double eps, int64_t step, double grad_scale, void *stream);

/* ---- optimiser ----------------------------------------------------------------------------------
 * torch.optim.Adam step as configured by RobustENeRF.configure_optimizers
 * (models/robust_e_nerf.py:782-813): L2-style weight decay (grad += wd*p), bias correction.
 * grad_scale multiplies the gradient first (1/world_size after an all-reduce SUM).
 * zero_grad != 0: the gradient buffer is cleared in the same pass. */
int ren_adam_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay,
                  int64_t step, float grad_scale, int32_t zero_grad, void *stream);

/* ---- optimiser state on the device (ABI 25) -- for a step captured in a hipGraph (engine.Trainer._graph_step), whose
 * launches cannot carry the step number as an argument, and whose optimiser must not run when a device-side sample count
 * (above) did not fit its arrays.  hyper = device double[8]: [REN_HY_STEP] Adam step of the float32 groups,
 * [REN_HY_SKIP] sticky skip word, [REN_HY_BC1/2] 1 - beta^step, [REN_HY_TAU_STEP], [REN_HY_TAU_BC1/2] the same for the
 * float64 group of the refractory period.  ren_step_tick: once per optimiser step, BEFORE its Adam launches -- raises skip
 * when the overflow words of stats_a / stats_b (int64[4] of ren_scan_guard: [1], [3]; either may be NULL) are set, otherwise
 * advances the step(s) and the corrections.  ren_adam_step_dev / ren_tau_adam_step_dev = ren_adam_step / ren_tau_adam_step
 * with the corrections from `hyper` (same arithmetic: robust_e_nerf.py:782-813); with skip raised they change NOTHING
 * (parameters, moments and gradients stay as they are: the host repeats the step and clears the word). */
#define REN_HY_STEP 0
#define REN_HY_SKIP 1
#define REN_HY_BC1 2
#define REN_HY_BC2 3
#define REN_HY_TAU_STEP 4
#define REN_HY_TAU_BC1 5
#define REN_HY_TAU_BC2 6
int ren_step_tick(double *hyper, double beta1, double beta2, const int64_t *stats_a, const int64_t *stats_b, int32_t tick_tau,
                  void *stream);
int ren_adam_step_dev(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                      float lr, float beta1, float beta2, float eps, float weight_decay,
                      const double *hyper, float grad_scale, int32_t zero_grad, void *stream);
int ren_tau_adam_step_dev(double *tau_raw, double *tau_grad, double *state, double tau_max, double lr, double beta1,
                          double beta2, double eps, const double *hyper, double grad_scale, void *stream);

/* ---- occupancy grid -------------------------------------------------------------------------------
 * nerfacc.OccupancyGrid._update as driven by NeRF.update_occ_grid (models/nerf.py:170-204). */
/* cell indices[m] (int64) + jitter[m,3] -> world positions x[m,3] (contract_inv) and
 * valid[m] (sphere contraction drops |x-0.5| >= 0.5).  roi host[6], res host[3]. */
int ren_occgrid_cell_points(const int64_t *indices, const float *jitter, int64_t m,
                            const float *roi_host, const int32_t *res_host,
                            int32_t contraction_type, float *x_world, uint8_t *valid, void *stream);
/* occs[idx] = max(occs[idx]*decay, sigma*step) for valid cells (models/nerf.py:197-198).
 * step_sizes[m] may be NULL (then `step_size` is used; cone_angle == 0). */
int ren_occgrid_ema(float *occs, const int64_t *indices, const uint8_t *valid, const float *sigma,
                    const float *step_sizes, float step_size, int64_t m, float ema_decay,
                    void *stream);
/* The same for cell samples that may hold duplicates (past warm-up nerfacc draws cells with replacement; its indexed
 * assignment keeps an arbitrary candidate): deterministic, a cell takes the largest of its new occupancies, decayed once.
 * scratch_cells: one float per grid cell (contents irrelevant). */
int ren_occgrid_ema_unique(float *occs, const int64_t *indices, const uint8_t *valid, const float *sigma,
                           const float *step_sizes, float step_size, int64_t m, float ema_decay, float *scratch_cells,
                           void *stream);
/* binary = occs > min(mean(occs), occ_thre);  scratch[2] device floats. */
int ren_occgrid_binarize(const float *occs, int64_t cells, float occ_thre, uint8_t *binary,
                         float *scratch, void *stream);

/* ---- forward-mode tangent path for the log-intensity-GRADIENT loss ---------------------------------
 * The reference computes d(log I)/d(timestamp) per ray with autograd.gradient(..., create_graph=True)
 * (robust_e_nerf/models/robust_e_nerf.py:383-409, utils/autograd.py:4-34) and back-propagates through
 * it.  Here every stage carries a tangent ("*d" arrays = d/dt, per unit of the timestamp) next to its
 * value, and the *_bwd_jvp entry points are the reverse pass over the (value, tangent) pair.  Sample
 * placement is not differentiated (external/vol_rendering.py:36-37).  Fragment layouts as above. */
/* LinearTrajectory.forward + d/dt: dpos[B,3], drot[B,9] */
int ren_trajectory_jvp(const double *ts, int64_t B, const int64_t *tab_ts, const float *tab_pos,
                       const float *tab_quat, int64_t C, float *pos, float *rot, float *dpos, float *drot,
                       void *stream);
/* pixel_params_to_ray + d/dt: rays_do[B,3], rays_dd[B,3] */
int ren_raygen_jvp(const float *Kinv, const float *px, const float *pos, const float *rot, const float *dpos,
                   const float *drot, int64_t B, float *rays_o, float *rays_d, float *rays_do, float *rays_dd,
                   void *stream);
/* hash features and their tangent (x = o + d tm, xd = od + dd tm) */
int ren_hashgrid_fwd_jvp(const ren_grid_desc *grid, const float *table, const ren_scene_desc *scene,
                         const float *rays_o, const float *rays_d, const float *rays_do, const float *rays_dd,
                         const int32_t *ray_indices, const float *t_starts, const float *t_ends, int64_t n,
                         float *feat, float *featd, const int64_t *n_dev, void *stream);
/* grad_table += w dfeat + wd dfeatd (per-update atomics) */
int ren_hashgrid_bwd_jvp(const ren_grid_desc *grid, float *grad_table, const ren_scene_desc *scene,
                         const float *rays_o, const float *rays_d, const float *rays_do, const float *rays_dd,
                         const int32_t *ray_indices, const float *t_starts, const float *t_ends, int64_t n,
                         const float *dfeat, const float *dfeatd, void *stream);
/* the same through the LDS-binned scatter (workspace as for ren_hashgrid_bwd_binned) */
int ren_hashgrid_bwd_binned_jvp(const ren_grid_desc *grid, float *grad_table, const ren_scene_desc *scene,
                                const float *rays_o, const float *rays_d, const float *rays_do,
                                const float *rays_dd, const int32_t *ray_indices, const float *t_starts,
                                const float *t_ends, int64_t n, const float *dfeat, const float *dfeatd,
                                void *workspace, void *stream);
/* Either of the two binned calls restricted to the levels whose bit is set in level_mask (rays_do / rays_dd / dfeatd all
 * NULL: value-only call; all given: the tangent call).  Data-parallel training (replaces DDP's bucketed
 * all-reduce of scripts/run.py:81-93) runs the fine levels first and all-reduces their slice of the table gradient while
 * the coarse levels are scattered. */
int ren_hashgrid_bwd_binned_levels(const ren_grid_desc *grid, float *grad_table, const float *x_unit,
                                   const ren_scene_desc *scene, const float *rays_o, const float *rays_d,
                                   const int32_t *ray_indices, const float *t_starts, const float *t_ends, int64_t n,
                                   int32_t layout, const float *dfeat, const float *rays_do, const float *rays_dd,
                                   const float *dfeatd, uint32_t level_mask, void *workspace, const int64_t *n_dev, void *stream);
/* The binned backward in phases: `begin` (clear, count, offsets -- needs the sample stream only), any number of `scatter`
 * calls over sample ranges [first, first + m) of the SAME stream (first on a 32-sample block; every call takes the whole
 * stream's n and pointers), and ONE `finish` (partition, accumulate, flush into grad_table).  Stream-ordered: begin before
 * every scatter, every scatter before finish -- the caller may run the scatters on another stream than whatever produces
 * the next range's dfeat (engine.py: MLP backward of chunk k + 1 beside the scatter of chunk k).  Same workspace and
 * results as ren_hashgrid_bwd_binned; replaces the tcnn backward at external/ngp.py:166-170. */
int ren_hashgrid_bwd_binned_begin(const ren_grid_desc *grid, const float *x_unit, const ren_scene_desc *scene,
                                  const float *rays_o, const float *rays_d, const int32_t *ray_indices,
                                  const float *t_starts, const float *t_ends, int64_t n, int32_t layout,
                                  void *workspace, void *stream);
int ren_hashgrid_bwd_binned_scatter(const ren_grid_desc *grid, float *grad_table, const float *x_unit,
                                    const ren_scene_desc *scene, const float *rays_o, const float *rays_d,
                                    const int32_t *ray_indices, const float *t_starts, const float *t_ends,
                                    int64_t n, int32_t layout, const float *dfeat, int64_t first, int64_t m,
                                    void *workspace, void *stream);
int ren_hashgrid_bwd_binned_finish(const ren_grid_desc *grid, float *grad_table, int64_t n, int32_t layout,
                                   void *workspace, void *stream);
/* fused MLPs with tangent: rgb, rgbd [n,C]; sigma, sigmad [n]; base_out, base_outd (ceil(n/32)*512 floats) */
int ren_mlp_fwd_jvp(const float *mlp_params, int32_t radiance_dim, int32_t activations, const float *feat, const float *featd,
                    const ren_scene_desc *scene, const float *rays_o, const float *rays_d, const float *rays_dd,
                    const int32_t *ray_indices, const float *t_starts, const float *t_ends, int64_t n,
                    float *rgb, float *rgbd, float *sigma, float *sigmad, float *base_out, float *base_outd,
                    void *stream);
int64_t ren_mlp_bwd_jvp_workspace_floats(int32_t radiance_dim);
/* reverse pass: (d_rgb, d_rgbd, d_sigma, d_sigmad) -> dfeat, dfeatd (fragment) and grad_mlp_params (+=).
 * scratch: ceil(n/32)*5120 floats; workspace: ren_mlp_bwd_jvp_workspace_floats() floats. */
int ren_mlp_bwd_jvp(const float *mlp_params, int32_t radiance_dim, int32_t activations, const float *feat, const float *featd,
                    const float *base_out, const float *base_outd, const ren_scene_desc *scene,
                    const float *rays_o, const float *rays_d, const float *rays_dd, const int32_t *ray_indices,
                    const float *t_starts, const float *t_ends, int64_t n, const float *rgb,
                    const float *d_rgb, const float *d_rgbd, const float *d_sigma, const float *d_sigmad,
                    float *scratch, float *dfeat, float *dfeatd, float *grad_mlp_params, float *workspace,
                    void *stream);
/* The same two calls on the bf16 matrix cores (csrc/ren_mlp_jvp_x.hip; default tangent path since ABI v15).
 * mode 6: split-bf16 products at fp32 accuracy (mode 3: two pieces, three products); mode 1: plain bf16 operands with fp32 accumulation for value AND tangent
 * of every nn.Linear (BASELINE configs[2]: bf16 MLP + fp32 composite with the log-intensity-gradient loss of
 * robust_e_nerf/models/robust_e_nerf.py:383-409 switched on).  Buffers, scratch and layouts as for the calls above. */
int ren_mlp_fwd_jvp_x(const float *mlp_params, int32_t radiance_dim, int32_t activations, int32_t mode, const float *feat, const float *featd,
                      const ren_scene_desc *scene, const float *rays_o, const float *rays_d, const float *rays_dd,
                      const int32_t *ray_indices, const float *t_starts, const float *t_ends, int64_t n,
                      float *rgb, float *rgbd, float *sigma, float *sigmad, float *base_out, float *base_outd,
                      const int64_t *n_dev, void *stream);
int64_t ren_mlp_bwd_jvp_x_workspace_floats(int32_t radiance_dim);
int ren_mlp_bwd_jvp_x(const float *mlp_params, int32_t radiance_dim, int32_t activations, int32_t mode, const float *feat, const float *featd,
                      const float *base_out, const float *base_outd, const ren_scene_desc *scene,
                      const float *rays_o, const float *rays_d, const float *rays_dd, const int32_t *ray_indices,
                      const float *t_starts, const float *t_ends, int64_t n, const float *rgb, const float *d_rgb,
                      const float *d_rgbd, const float *d_sigma, const float *d_sigmad, float *scratch, float *dfeat,
                      float *dfeatd, float *grad_mlp_params, float *workspace, const int64_t *n_dev, void *stream);
/* compositing with tangent: colors/colords [n_rays,C], opacities/opacds [n_rays]; saves weights, trans,
 * eds (exclusive prefix of sigmad*dt) [n] for the reverse pass */
int ren_composite_fwd_jvp(const int64_t *offsets, const int32_t *counts, int64_t n_rays, const float *t_starts,
                          const float *t_ends, const float *sigmas, const float *sigmads, const float *rgbs,
                          const float *rgbds, int32_t C, const float *bkgd, float *colors, float *colords,
                          float *opacities, float *opacds, float *weights, float *trans, float *eds, void *stream);
int ren_composite_bwd_jvp(const int64_t *offsets, const int32_t *counts, int64_t n_rays, const float *t_starts,
                          const float *t_ends, const float *sigmas, const float *sigmads, const float *rgbs,
                          const float *rgbds, int32_t C, const float *bkgd, const float *weights,
                          const float *trans, const float *eds, const float *opacities, const float *opacds,
                          const float *g_colors, const float *g_colords, float *d_sigmas, float *d_sigmads,
                          float *d_rgbs, float *d_rgbds, float *d_bkgd_per_ray, void *stream);
/* Epilogue of the tangent (l_grad) render in one launch (robust_e_nerf.py:390-398,865-871, `bayering` :887-890):
 * intensity = colors[:, channel] + min_modeled_intensity, intensity_dot = colords[:, channel], valid = opacity > 0 (NULL:
 * a background parameter makes every ray valid), dlog_dt = intensity_dot / intensity (NULL: not wanted).  C = 1: channel_idx
 * may be NULL. */
int ren_rate_epilogue(const float *colors, const float *colords, const float *opacities, const uint8_t *channel_idx,
                      int32_t C, int64_t n, float min_modeled_intensity, float *intensity, float *intensity_dot,
                      uint8_t *valid, float *dlog_dt, void *stream);
/* d loss / d tau through the poses (robust_e_nerf.py:340-357: tau moves every supervision timestamp):
 * tau_grad[0] += sum_i (g_a[i] x_a[i] + g_b[i] x_b[i]) dts[i], float64, one launch (g_b, x_b may both be NULL). */
int ren_tau_pose_grad(const float *g_a, const float *x_a, const float *g_b, const float *x_b, const double *dts,
                      int64_t n, double *tau_grad, void *stream);
/* torch.nn.utils.weight_norm(module) over the Linear layers of an MLP (external/ngp.py:207-228, external/mlp.py:303-319;
 * dim 0): W[r, :] = g[r] v[r, :] / ||v[r, :]||.  `raw` is the packed parameter block with v in the weight slots, `eff` the
 * block the field kernels read; `layers` (HOST memory) lists the reparametrised weights as n_layers x {weight offset, rows,
 * cols, offset of the layer's first g in `g`} (<= 16 layers); every other element of the block is copied through.
 * _bwd: d_raw = gradient w.r.t. (v, biases, plain weights) from d_eff = gradient w.r.t. the effective block, d_g[r] =
 * dW[r, :] . v / ||v||; zero_d_eff != 0 clears d_eff afterwards (the accumulator of the next step).  Two small launches each. */
int ren_weight_norm_fwd(const float *raw, const float *g, const int32_t *layers, int32_t n_layers, int64_t n_params,
                        float *eff, void *stream);
int ren_weight_norm_bwd(const float *raw, const float *g, float *d_eff, const int32_t *layers, int32_t n_layers,
                        int64_t n_params, float *d_raw, float *d_g, int32_t zero_d_eff, void *stream);
/* Loss.log_intensity_grad (loss_metric/loss.py:43-57): pred = intensity_dot / intensity vs target;
 * same loss_sum / scale conventions as ren_event_loss_fwd/bwd */
int ren_grad_loss_fwd(const float *intensity, const float *intensity_dot, const float *target,
                      const uint8_t *valid, int64_t B, int32_t err_fn, float *loss_sum, void *stream);
int ren_grad_loss_bwd(const float *intensity, const float *intensity_dot, const float *target,
                      const uint8_t *valid, int64_t B, int32_t err_fn, float scale, const double *scale_dev,
                      const float *loss_sum, float *g_intensity, float *g_intensity_dot, float *loss, void *stream);
/* scale_dev: as for ren_event_diff_loss_bwd; loss (may be NULL): loss[0] = scale * loss_sum[0] / loss_sum[1] */

/* ---- bf16 MLP mode (BASELINE configs[2]: "bf16 MLP with fp32 composite") ------------------------------ *
 * Same arguments as ren_mlp_fwd / ren_mlp_bwd.  Every linear layer sees bf16-rounded (nearest-even) inputs;
 * `mlp_params_bf16` is the caller's bf16-rounded copy of the parameter block (still f32 storage); products
 * accumulate in fp32, bias and activations stay fp32.  The backward is the exact derivative of that forward
 * (straight-through rounding) and accumulates into the fp32 master gradient. */
int ren_mlp_fwd_bf16(const float *mlp_params_bf16, int32_t C, int32_t activations, const float *feat, const ren_scene_desc *scene,
                     const float *x_world, const float *dirs, const float *rays_o, const float *rays_d,
                     const int32_t *ray_indices, const float *t_starts, const float *t_ends, int64_t n,
                     int32_t density_only, float *rgb, float *sigma, float *base_out, void *stream);
int ren_mlp_bwd_bf16(const float *mlp_params_bf16, int32_t C, int32_t activations, const float *feat, const float *base_out,
                     const ren_scene_desc *scene, const float *x_world, const float *dirs, const float *rays_o,
                     const float *rays_d, const int32_t *ray_indices, const float *t_starts,
                     const float *t_ends, int64_t n, const float *rgb, const float *d_rgb, const float *d_sigma,
                     float *d_base, float *dfeat, float *grad_mlp_params, float *workspace, void *stream);

/* ---- saved-activation variants (the training fast path) -------------------------------------------------- *
 * ren_mlp_fwd_save additionally stores the post-activation values of the three hidden layers
 * (ren_mlp_act_save_floats(n) floats, 768 B/sample); ren_mlp_bwd_saved reads them instead of recomputing
 * the forward (128 f32 MFMAs + 192 softplus per 32 samples).  bf16 != 0 selects the bf16 numerics mode
 * (mlp_params is then the rounded copy).  Otherwise the arguments of ren_mlp_fwd / ren_mlp_bwd. */
int64_t ren_mlp_act_save_floats(int64_t n);
int ren_mlp_fwd_save(const float *mlp_params, int32_t C, int32_t activations, int32_t bf16, const float *feat,
                     const ren_scene_desc *scene, const float *x_world, const float *dirs, const float *rays_o,
                     const float *rays_d, const int32_t *ray_indices, const float *t_starts,
                     const float *t_ends, int64_t n, float *rgb, float *sigma, float *base_out, float *act_save,
                     void *stream);
int ren_mlp_bwd_saved(const float *mlp_params, int32_t C, int32_t activations, int32_t bf16, const float *feat, const float *base_out,
                      const float *act_save, const ren_scene_desc *scene, const float *x_world, const float *dirs,
                      const float *rays_o, const float *rays_d, const int32_t *ray_indices, const float *t_starts,
                      const float *t_ends, int64_t n, const float *rgb, const float *d_rgb, const float *d_sigma,
                      float *d_base, float *dfeat, float *grad_mlp_params, float *workspace, void *stream);

/* ---- split-bf16 MLP kernels (csrc/ren_mlp_x.hip) ------------------------------------------------------------- *
 * The same fused MLPs on the bf16 matrix cores.  mode 6: every fp32 operand is split exactly into three bf16
 * pieces and six bf16 MFMAs per k-chunk reproduce the fp32 product to fp32 round-off (the default training
 * path: the f32 MFMA shares its pipe with the VALU on gfx950, the bf16 MFMA does not).  mode 1: plain bf16
 * operands (BASELINE configs[2]); takes the fp32 parameter block and rounds it itself.  mode 3: two bf16 pieces per
 * operand and three products a1 b2 + a2 b1 + a1 b1 -- "each float32 number as the sum of two bfloat16 numbers", i.e.
 * `float32_matmul_precision: high` of the reference's YAMLs (scripts/run.py:34-35): ~16 significant bits per product,
 * half of mode 6's matrix-pipe time.  The same three modes for the *_jvp_x / *_jvp2_x entry points.
 * Arguments as ren_mlp_fwd_save / ren_mlp_bwd_saved; act_save may be NULL in the forward (inference).
 * flags: REN_MLP_DENSITY_ONLY (base network and sigma only; rgb may be NULL), REN_MLP_SHARE_CU (one persistent
 * workgroup per CU instead of two, leaving half of each CU to a kernel running on another stream: the engine
 * runs the hash encoding of the next sample chunk beside the MLP of the current one). */
#define REN_MLP_DENSITY_ONLY 1
#define REN_MLP_SHARE_CU 2
int ren_mlp_fwd_x(const float *mlp_params, int32_t C, int32_t activations, int32_t mode, const float *feat, const ren_scene_desc *scene,
                  const float *x_world, const float *dirs, const float *rays_o, const float *rays_d,
                  const int32_t *ray_indices, const float *t_starts, const float *t_ends, int64_t n,
                  int32_t flags, float *rgb, float *sigma, float *base_out, float *act_save, const int64_t *n_dev, void *stream);
int64_t ren_mlp_bwd_x_workspace_floats(int32_t C);
int ren_mlp_bwd_x(const float *mlp_params, int32_t C, int32_t activations, int32_t mode, const float *feat, const float *base_out,
                  const float *act_save, const ren_scene_desc *scene, const float *x_world, const float *dirs,
                  const float *rays_o, const float *rays_d, const int32_t *ray_indices, const float *t_starts,
                  const float *t_ends, int64_t n, const float *rgb, const float *d_rgb, const float *d_sigma,
                  float *d_base, float *dfeat, float *grad_mlp_params, float *workspace, int32_t grid_cus, const int64_t *n_dev, void *stream);
/* grid_cus: persistent workgroups (= CUs) the two backward kernels occupy, 1 .. 255; 0 (or >= 256) = all 256.  The chunked
 * backward of engine.py lowers it while a scatter runs on the second stream (until ABI 23: knob REN_KNOB_MLP_BWD_CUS). */

/* ---- second-order forward tangent (value, d/dt, d2/dt2): d(l_grad)/d(tau) --------------------------- *
 * The gradient-loss prediction d(log I)/dt is evaluated at ts_g(tau); its derivative w.r.t. the refractory
 * period needs d2 I/dt2 per ray (models/robust_e_nerf.py:340-357,383-409 differentiated through
 * `grad.ts`; the reference obtains it as a third-order autograd graph).  Forward only, same sample
 * stream as the first-order render.  Arrays with suffix dd hold second time derivatives. */
int ren_trajectory_jvp2(const double *ts, int64_t B, const int64_t *tab_ts, const float *tab_pos,
                        const float *tab_quat, int64_t C, float *pos, float *rot, float *dpos, float *drot,
                        float *ddrot, void *stream);
int ren_raygen_jvp2(const float *Kinv, const float *px, const float *pos, const float *rot, const float *dpos,
                    const float *drot, const float *ddrot, int64_t B, float *rays_o, float *rays_d,
                    float *rays_do, float *rays_dd, float *rays_ddd, void *stream);
int ren_hashgrid_fwd_jvp2(const ren_grid_desc *grid, const float *table, const ren_scene_desc *scene,
                          const float *rays_o, const float *rays_d, const float *rays_do, const float *rays_dd,
                          const float *rays_ddd, const int32_t *ray_indices, const float *t_starts,
                          const float *t_ends, int64_t n, float *feat, float *featd, float *featdd, const int64_t *n_dev,
                          void *stream);
int ren_mlp_fwd_jvp2(const float *mlp_params, int32_t C, int32_t activations, const float *feat, const float *featd,
                     const float *featdd, const ren_scene_desc *scene, const float *rays_o, const float *rays_d,
                     const float *rays_do, const float *rays_dd, const float *rays_ddd,
                     const int32_t *ray_indices, const float *t_starts, const float *t_ends, int64_t n,
                     float *rgb, float *rgbd, float *rgbdd, float *sigma, float *sigmad, float *sigmadd,
                     void *stream);
/* ren_mlp_fwd_jvp2 on the bf16 matrix cores (csrc/ren_jvp2.hip: mlp_fwd_jvp2_x_kernel); mode 6: split-bf16 at fp32
 * accuracy (3: two pieces, three products), mode 1: plain bf16 operands -- the second-order render of a step follows the precision mode of its other
 * MLP kernels (RenderCfg.mlp_kernels = "x") */
int ren_mlp_fwd_jvp2_x(const float *mlp_params, int32_t C, int32_t activations, int32_t mode, const float *feat, const float *featd,
                       const float *featdd, const ren_scene_desc *scene, const float *rays_o, const float *rays_d,
                       const float *rays_do, const float *rays_dd, const float *rays_ddd,
                       const int32_t *ray_indices, const float *t_starts, const float *t_ends, int64_t n,
                       float *rgb, float *rgbd, float *rgbdd, float *sigma, float *sigmad, float *sigmadd,
                       const int64_t *n_dev, void *stream);
int ren_composite_fwd_jvp2(const int64_t *offsets, const int32_t *counts, int64_t n_rays, const float *t_starts,
                           const float *t_ends, const float *sigmas, const float *sigmads, const float *sigmadds,
                           const float *rgbs, const float *rgbds, const float *rgbdds, int32_t C,
                           const float *bkgd, float *colors, float *colords, float *colorsdd, void *stream);

/* ---- vanilla-NeRF field, `arch: mlp` (external/mlp.py:26-113,126-205,208-243,246-358) ----------------- *
 * Activations are row-major [n_pad][ld] f32, n_pad = n rounded up to 32, ld a multiple of 4 and at least
 * the layer width rounded up to 32, padding columns ZERO (they are read as part of the reduction).
 * Concatenations are column ranges of one buffer.  Weights are torch nn.Linear [n_out][n_in] + bias. */
#define REN_ACT_NONE 0
#define REN_ACT_SOFTPLUS100 1          /* Softplus(beta=100), models/nerf.py:17-29          */
#define REN_ACT_SOFTPLUS1 2            /* Softplus(beta=1)                                  */
#define REN_ACT_TRUNC_EXP_SEL 3        /* selector * exp(z - 1), external/ngp.py:45-65, mlp.py:343 */
/* the YAML's alternatives (models/nerf.py:8-29); backward-data takes REN_ACT_RELU as a previous-layer activation too.  The
 * output-head kernels of arch mlp (ren_vanilla_heads_*) differentiate the density / radiance kinds of REN_KNOB_ACTIVATIONS;
 * the tangent algebra (ren_act_jvp*) takes beta = 0 for relu.  The fused field (ren_vanilla_fwd / _bwd) implements the
 * shipped set only and returns REN_ERR_UNSUPPORTED under a non-zero REN_KNOB_ACTIVATIONS. */
#define REN_ACT_RELU 4
#define REN_ACT_SIGMOID 5
#define REN_ACT_SOFTPLUS1_SEL 6        /* selector * softplus(z)                            */
#define REN_ACT_SHIFTED_SOFTPLUS1_SEL 7 /* selector * softplus(z - 1), models/nerf.py:8-13  */
/* SinusoidalEncoder of the contracted position (63 features -> enc[:, :64], col 63 = 0; optional copy at
 * cat[:, cat_col:cat_col+64]) and of pi*direction (27 features, padded to 32, at view[:, view_col:]);
 * selector[i] = all(0 < contracted x < 1).  Positions from x_world/dirs or from the packed sample stream. */
int ren_freq_encode(const ren_scene_desc *scene, const float *x_world, const float *dirs, const float *rays_o,
                    const float *rays_d, const int32_t *ray_indices, const float *t_starts,
                    const float *t_ends, int64_t n, float *enc, int32_t ld_enc, float *cat, int32_t ld_cat,
                    int32_t cat_col, float *view, int32_t ld_view, int32_t view_col, uint8_t *selector,
                    void *stream);
/* Y[:, :n_out] = act(X[:, :n_in] W^T + b)  (nn.Linear + activation, mlp.py:99-113), n_out <= 256
 * Matrix-core path: OR one of these into `act` (ren_dense_fwd) / `prev_act` (ren_dense_bwd_data):
 * REN_DENSE_F32 exact v_mfma_f32_32x32x2_f32; REN_DENSE_BF16X6 split-bf16, six bf16 MFMAs per k-step at fp32
 * accuracy (2.7x fewer matrix-pipe cycles, co-issues with the VALU); REN_DENSE_BF16 plain bf16 operands. */
#define REN_DENSE_F32 0x000
#define REN_DENSE_BF16X6 0x600
#define REN_DENSE_BF16 0x100
int ren_dense_fwd(const float *X, int32_t ldx, const float *W, const float *bias, int32_t n_out, int32_t n_in,
                  int32_t act, const uint8_t *selector, float *Y, int32_t ldy, int64_t n, void *stream);
/* dX[:, :n_store] (+)= dZ[:, :n_out] W[:, :n_store], then multiplied by prev_act'(Yprev) -> the dZ of the
 * layer below (n_store <= n_in: gradients of concatenated encodings are not needed) */
int ren_dense_bwd_data(const float *dZ, int32_t ldz, const float *W, int32_t n_out, int32_t n_in, int32_t n_store,
                       int32_t prev_act, const float *Yprev, int32_t ldyp, int32_t accumulate, float *dX,
                       int32_t ldx, int64_t n, void *stream);
/* grad_w[n_out][n_in] += dZ^T X, grad_b[n_out] += column sums of dZ (slab-reduced, deterministic); grad_b may be NULL
 * (tangent stream of a layer: no bias) */
/* Activation algebra of the tangent stream of a dense layer (log-intensity-gradient loss with arch mlp): y = softplus_beta(z),
 * yd = s zd with s = 1 - exp(-beta y) taken from the output.  fwd: Yd = s Zd.  bwd: gz = gy s + gyd zd beta s (1 - s),
 * gzd = gyd s.  Row-major buffers; Y (and Yd in fwd) may be column ranges of wider buffers (ld), the others are dense
 * [rows][width]; width and every ld are multiples of 4. */
int ren_act_jvp_fwd(const float *Y, int32_t ldy, const float *Zd, int32_t ldz, float beta, float *Yd, int32_t ldyd,
                    int64_t rows, int32_t width, void *stream);
int ren_act_jvp_bwd(const float *gy, const float *gyd, const float *Y, int32_t ldy, const float *Zd, float beta, float *gz,
                    float *gzd, int64_t rows, int32_t width, void *stream);
int64_t ren_dense_bwd_weight_workspace_floats(int32_t n_out, int32_t n_in, int32_t n_splits);
/* Matrix-core path of ren_dense_bwd_weight: OR (REN_DENSE_BF16X6 or REN_DENSE_BF16) << 8 into n_splits (bits 16..23) for
 * bf16 MFMAs: REN_DENSE_BF16X6 = operands split into three bf16 pieces, six MFMAs per product pair (fp32 round-off);
 * REN_DENSE_BF16 = plain bf16 operands (one MFMA); default: exact f32 MFMA. */
int ren_dense_bwd_weight(const float *dZ, int32_t ldz, const float *X, int32_t ldx, int32_t n_out, int32_t n_in,
                         int64_t n, int32_t n_splits, float *grad_w, float *grad_b, float *workspace,
                         void *stream);
/* output activations backward: dz_rgb[n_pad][32] = g_rgb * softplus1'(rgb), dz_sigma[n_pad][32] (col 0) =
 * g_sigma * d sigma/d raw; padding zeroed */
int ren_vanilla_heads_bwd(const float *g_rgb, const float *rgb, const float *g_sigma, const float *sigma,
                          int64_t n, int32_t C, int32_t activations, float *dz_rgb, float *dz_sigma, void *stream);

/* ---- arch mlp: the whole field as one launch per pass (csrc/ren_vfield.hip) ------------------------------------------------
 * Replaces NerfMLP.forward / query_density (robust_e_nerf/external/mlp.py:126-205: eight hidden Linear + Softplus(beta = 100)
 * with the skip concatenation after layer 4, sigma layer, bottleneck, 283 -> 128 -> C colour head) and its autograd:
 * activations stay in registers from layer to layer.  `params`: the field's parameter block (reference state-dict order,
 * torch layout).  `mode`: REN_DENSE_BF16 (1: bf16 operands, saved copies in bf16), REN_DENSE_BF16X6 (6: three-piece split,
 * fp32 round-off, saved copies in fp32) or 3 (two pieces, three products = `float32_matmul_precision: high`; layouts of
 * mode 6, an image of two pieces; every ren_vanilla_* entry point, not the per-layer ren_dense_* ones).  `image` (ren_vanilla_image_bytes) is the MFMA-fragment form of the weights: rebuild
 * it with ren_vanilla_prep whenever the parameters change.  `saved` / `dz` (ren_vanilla_saved_bytes each) hold the layers'
 * activations / pre-activation gradients in the kernels' fragment layout (documented in ren_vfield.hip).
 * fwd: enc [n_pad][ld_enc >= 64], view [n_pad][ld_view >= 32], selector [n_pad] are the outputs of ren_freq_encode (rows
 * n .. n_pad zero); sigma [n_pad]; rgb4 [n_pad][4] (columns >= C zero) or NULL for the density only (then view may be NULL
 * and saved must be).  bwd: dz_rgb / dz_sigma [n_pad][32] as written by ren_vanilla_heads_bwd.  ren_vanilla_bwd_weight ADDS
 * dW_l = dz_l^T x_{l-1}, db_l = sum dz_l of all twelve layers to `grads` (layout of params), slab-reduced (deterministic).
 * Backward over a sample RANGE of a larger forward pass (bounds the memory of `dz`): row pointers (dz_rgb, dz_sigma, enc, view)
 * and `saved` advanced to the first sample of the range -- a multiple of 256 samples; saved + first_sample * 256 * element
 * size -- n = samples in the range, saved_slot_bytes = ren_vanilla_saved_bytes(mode, n_forward) / 10 (0: the pass itself). */
int64_t ren_vanilla_image_bytes(int32_t mode);
int64_t ren_vanilla_saved_bytes(int32_t mode, int64_t n);
int ren_vanilla_prep(const float *params, int32_t C, int32_t mode, void *image, void *stream);
int ren_vanilla_fwd(const float *enc, int32_t ld_enc, const float *view, int32_t ld_view, const uint8_t *selector,
                    const float *params, int32_t C, int32_t activations, const void *image, int32_t mode, int64_t n, void *saved, float *sigma,
                    float *rgb4, void *stream);
int ren_vanilla_bwd(const float *dz_rgb, const float *dz_sigma, const void *image, int32_t mode, int32_t activations, int64_t n, const void *saved,
                    int64_t saved_slot_bytes, void *dz, void *stream);
/* Value + forward-mode tangent (d/dt) of the whole field in one launch each way -- the third render of the step with the
 * log-intensity-gradient loss (models/robust_e_nerf.py:383-409 through external/mlp.py:126-205 under utils/autograd.py:4-34).
 * REN_DENSE_BF16: value and tangent are the two 32-sample "blocks" of a wave, one launch each way.  REN_DENSE_BF16X6 (fp32
 * round-off): two launches each way -- forward: the value, then the tangent with sp'(z) from the value's saved copies (saved
 * is required); reverse: the tangent side, which leaves its coupling term per layer in `coupling` (ren_vanilla_saved_bytes,
 * required in this mode), then the value side.  Other modes / activation sets: REN_ERR_UNSUPPORTED (per-layer launches).  encd / viewd:
 * d/dt of the two encodings (ren_freq_encode_jvp, same leading dimensions as enc / view); saved / savedd: the layers' value /
 * tangent activations (ren_vanilla_saved_bytes each; both or neither); zsd4 / zod4 [n_pad][4]: tangent pre-activations of the
 * sigma head (column 0) and the colour head (columns < C) for ren_vanilla_heads_jvp / ren_vanilla_heads_bwd_jvp.  bwd_jvp: the
 * four [n_pad][32] gradient buffers of ren_vanilla_heads_bwd_jvp -> dz / dzd (ren_vanilla_saved_bytes each).  The weight
 * gradients are ren_vanilla_bwd_weight(dz, saved, ..) + ren_vanilla_bwd_weight_tangent(dzd, savedd, .., encd, viewd, dzd_rgb,
 * dzd_sigma, ..): the latter adds dW_l += dzd_l^T xd_(l-1) only (the tangent stream has no bias). */
int ren_vanilla_fwd_jvp(const float *enc, int32_t ld_enc, const float *view, int32_t ld_view, const float *encd, const float *viewd,
                        const uint8_t *selector, const float *params, int32_t C, int32_t activations, const void *image, int32_t mode,
                        int64_t n, void *saved, void *savedd, float *sigma, float *rgb4, float *zsd4, float *zod4, void *stream);
int ren_vanilla_bwd_jvp(const float *dz_rgb, const float *dzd_rgb, const float *dz_sigma, const float *dzd_sigma, const void *image,
                        int32_t mode, int32_t activations, int64_t n, const void *saved, const void *savedd, int64_t saved_slot_bytes,
                        void *dz, void *dzd, void *coupling, void *stream);
int ren_vanilla_bwd_weight_tangent(const void *dzd, const void *savedd, int64_t saved_slot_bytes, const float *encd, int32_t ld_enc,
                                   const float *viewd, int32_t ld_view, const float *dzd_rgb, const float *dzd_sigma, int32_t C,
                                   int32_t mode, int64_t n, int32_t n_splits, float *grads, float *workspace, void *stream);
int64_t ren_vanilla_bwd_weight_workspace_floats(int32_t n_splits);
int ren_vanilla_bwd_weight(const void *dz, const void *saved, int64_t saved_slot_bytes, const float *enc, int32_t ld_enc,
                           const float *view, int32_t ld_view, const float *dz_rgb, const float *dz_sigma, int32_t C,
                           int32_t mode, int64_t n, int32_t n_splits, float *grads, float *workspace, void *stream);
/* Tangent streams of the vanilla field (robust_e_nerf/external/mlp.py:208-243,333-358 under
 * utils/autograd.py:4-34 for the log-intensity-gradient loss, models/robust_e_nerf.py:383-409; the second order serves
 * d loss / d tau, see ren_trajectory_jvp2).  ren_freq_encode_jvp: `order`-th time derivative (1 or 2) of ren_freq_encode's
 * position / view features for a packed sample stream whose rays carry o, d and their time derivatives do, dd, ddd
 * (o'' = 0 inside a pose segment); same destinations and layout as ren_freq_encode, rows n..n_pad written as zeros. */
int ren_freq_encode_jvp(const ren_scene_desc *scene, const float *rays_o, const float *rays_d, const float *rays_do,
                        const float *rays_dd, const float *rays_ddd, const int32_t *ray_indices, const float *t_starts,
                        const float *t_ends, int64_t n, int32_t order, float *enc, int32_t ld_enc, float *cat, int32_t ld_cat,
                        int32_t cat_col, float *view, int32_t ld_view, int32_t view_col, void *stream);
/* y = softplus_beta(z) with first and second time derivatives: Yd = s Zd, Ydd = beta s (1 - s) Zd^2 + s Zdd */
int ren_act_jvp2_fwd(const float *Y, int32_t ldy, const float *Zd, const float *Zdd, int32_t ldz, float beta, float *Yd,
                     int32_t ldyd, float *Ydd, int32_t ldydd, int64_t rows, int32_t width, void *stream);
/* Output heads of the tangent streams: rgb = softplus_1(zo), sigma = selector exp(zs - 1) (clamped derivative, ngp.py:45-65).
 * zod / zodd / zsd / zsdd: [n_pad][4] pre-activation tangents (ren_dense_fwd without bias / activation); the second-order
 * arguments (zodd, zsdd, rgbdd, sigmadd) may all be NULL.  rgb* are (n, C), sigma* (n). */
int ren_vanilla_heads_jvp(const float *rgb, const float *sigma, const float *zod, const float *zodd, const float *zsd,
                          const float *zsdd, int64_t n, int32_t C, int32_t activations, float *rgbd, float *rgbdd, float *sigmad, float *sigmadd,
                          void *stream);
/* reverse pass of (rgb, rgbd, sigma, sigmad) -> pre-activation gradients of the value and the tangent stream, each
 * [n_pad][32] zero-padded (as ren_vanilla_heads_bwd) */
int ren_vanilla_heads_bwd_jvp(const float *g_rgb, const float *g_rgbd, const float *g_sigma, const float *g_sigmad,
                              const float *rgb, const float *sigma, const float *zod, const float *zsd, int64_t n, int32_t C, int32_t activations,
                              float *dz_rgb, float *dzd_rgb, float *dz_sigma, float *dzd_sigma, void *stream);

/* ---- evaluation metrics (csrc/ren_metrics.hip) ------------------------------------------------------- *
 * SSIM as the reference's validation / test epochs score every aligned view (loss_metric/metric.py:74-81: torchmetrics
 * ssim, 11 x 11 Gaussian window of sigma 1.5, k1 = 0.01, k2 = 0.03, data_range = the target's largest pixel value; the
 * epoch value is the mean over the views, robust_e_nerf.py:684-696).  A plane is one (view, channel) image: pred / target
 * are contiguous (P, H, W) float32 and out[p] (float64) is the mean SSIM over plane p's (H - 10) x (W - 10) valid windows --
 * torchmetrics reflect-pads by 5, filters and crops 5 pixels per border, so the padding never reaches the mean.  Moments
 * are filtered in fp64.  One launch scores all planes; deterministic (no atomics), repeated calls are bitwise equal.
 * REN_ERR_BAD_ARG for a null pointer, P < 1, H or W < 11 (no valid window) or a data_range that is not finite and > 0.
 * scratch: ren_ssim_scratch_doubles(P, H, W) doubles of device memory (0 for a shape that has no valid window). */
int64_t ren_ssim_scratch_doubles(int64_t P, int32_t H, int32_t W);
int ren_ssim_planes(const float *pred, const float *target, int64_t P, int32_t H, int32_t W, double data_range,
                    double *out, double *scratch, void *stream);

/* ---- event frames (csrc/ren_event_frames.hip) -------------------------------------------------------- *
 * Recorded events against the model's predicted brightness change: between the times edges[v] and edges[v + 1] pixel u saw
 * n+ positive and n- negative events, and the sensor model says log I(u, t1) - log I(u, t0) ~ c_p n+ - c_n n- to within one
 * threshold.  ren_event_frames bins the raw stream as raw_events.npz stores it -- position: N words x | y << 16 (an (N, 2)
 * uint16 array read as one 32-bit word per event), timestamp: N int64 nanoseconds in time order, polarity: N bytes, non-zero
 * = positive -- into counts, int32 (V, 2, H, W), plane 0 the positives and plane 1 the negatives.  The CALLER zeroes counts;
 * the call adds to it.  Event e belongs to window v iff edges[v] <= timestamp[e] < edges[v + 1] (edges: V + 1 int64 on the
 * device, non-decreasing -- not checked here; among equal edges the window before them is empty); events before edges[0], at
 * or after edges[V], or with x >= W or y >= H are dropped.  The window is found by a binary search per event, over a copy of
 * the edges in LDS while V + 1 <= REN_EVENT_FRAMES_LDS_EDGES and over global memory above that.  Integer atomics: the sums
 * are exact and independent of arrival order, repeated calls are bitwise equal.  flags: 0, or REN_EVENT_FRAMES_MERGE -- the
 * lanes of a wave that add to one counter are merged into one atomic (same result).
 * REN_ERR_BAD_ARG for a null edges / counts, a null event array with N > 0, N < 0, V < 1, H * W == 0 or an unknown flag,
 * before any launch; N == 0 launches nothing. */
#define REN_EVENT_FRAMES_LDS_EDGES 4096
#define REN_EVENT_FRAMES_MERGE 1
int ren_event_frames(const uint32_t *position, const int64_t *timestamp, const uint8_t *polarity, int64_t N,
                     const int64_t *edges, int32_t V, int32_t H, int32_t W, int32_t flags, int32_t *counts, void *stream);
/* Per-window comparison of the measured change m = c_p n+ - c_n n- (formed in fp64 from counts) with pred, float32 (V, H, W),
 * over the pixels with valid (uint8 (V, H, W)) != 0: out, float64 (V, 9) =
 *   [count, sum m, sum p, sum m^2, sum p^2, sum m p, sum (p - m)^2, #{|p - m| <= max(c_p, c_n)}, #{n+ + n- > 0}].
 * Two launches (tile partials, then a fixed-order sum per window), no float atomics: bitwise repeatable.
 * scratch: ren_event_frame_compare_scratch_doubles(V, H, W) doubles of device memory (0 for V < 1 or H * W == 0).
 * REN_ERR_BAD_ARG for a null pointer, V < 1, H * W == 0 or a c_p / c_n that is not finite. */
int64_t ren_event_frame_compare_scratch_doubles(int32_t V, int32_t H, int32_t W);
int ren_event_frame_compare(const int32_t *counts, const float *pred, const uint8_t *valid, int32_t V, int32_t H, int32_t W,
                            double c_p, double c_n, double *out, double *scratch, void *stream);

/* ---- event table (csrc/ren_event_table.hip) ---------------------------------------------------------- *
 * raw_events.npz -> the training's event table (data/datasets.py:133-364: per-pixel intervals, Bayer channel, undistorted
 * position) and tau_max (the minimum interval), device-resident, after ONE stable sort of the pixel keys by the caller.
 * ren_event_intervals: pix_sorted: N int32 keys y * W + x in stable by-pixel order; order: N int64, the stream index of each
 * sorted slot (a permutation of 0 .. N - 1); timestamp: N int64 in stream order.  For sorted slot i with j = order[i]:
 * valid[j] = (i > 0 and pix_sorted[i] == pix_sorted[i - 1] and d != 0) with d = timestamp[j] - timestamp[order[i - 1]] -- the
 * IMMEDIATE predecessor, kept or not -- and start_ts[j] = timestamp[order[i - 1]] where valid (other start_ts are not
 * written).  *min_diff (one int64 on the device, set to INT64_MAX by the CALLER) becomes min(*min_diff, d over the valid
 * slots): per wave, per workgroup, then one 64-bit atomic min per workgroup; bitwise repeatable.  An order entry outside
 * [0, N) is skipped.
 * ren_event_table_write: valid (N uint8) and offsets (N int32, the EXCLUSIVE prefix sum of valid) in stream order; position:
 * (N, 2) (x, y) as the file stores it, position_bytes = 2 (uint16), 4 (int32) or 8 (int64) per coordinate; polarity: N bytes;
 * M = sum of valid = rows of the outputs.  Kept event e writes row offsets[e]: out_position (M, 2) float32 = lut[y * W + x]
 * (lut: (H * W, 2) float32, NULL = the coordinates cast to float32; a pixel outside W x H is cast as well, the CALLER checks
 * the range), out_start_ts = start_ts[e], out_end_ts = timestamp[e], out_num_pos = polarity[e], out_num_neg = 1 -
 * polarity[e] (int64 each), out_channel_idx (uint8) = bayer_channels[(x & 1) + 2 * (y & 1)] (bayer_channels: 4 bytes on the
 * HOST in tile order TL, TR, BL, BR; NULL together with out_channel_idx for a monochrome sensor).  Rows keep stream order.
 * Both: grid-stride loops, no workgroup waits on another.  REN_ERR_BAD_ARG for a null or misaligned required pointer, a
 * negative size, M > N, H or W < 1, a position_bytes other than 2 / 4 / 8, or one of bayer_channels / out_channel_idx
 * without the other, before any launch; REN_ERR_UNSUPPORTED for N or H * W >= 2^31; N == 0 or M == 0 launches nothing. */
#define REN_EVENT_TABLE_THREADS 256          /* workgroup size of both kernels (at most 2 048 workgroups, grid-stride) */
int ren_event_intervals(const int32_t *pix_sorted, const int64_t *order, const int64_t *timestamp, int64_t N, uint8_t *valid,
                        int64_t *start_ts, int64_t *min_diff, void *stream);
int ren_event_table_write(const uint8_t *valid, const int32_t *offsets, const void *position, int32_t position_bytes,
                          const int64_t *timestamp, const int64_t *start_ts, const uint8_t *polarity, int64_t N, int64_t M,
                          const float *lut, int32_t H, int32_t W, const uint8_t *bayer_channels, float *out_position,
                          int64_t *out_start_ts, int64_t *out_end_ts, int64_t *out_num_pos, int64_t *out_num_neg,
                          uint8_t *out_channel_idx, void *stream);

/* ---- event filter (csrc/ren_event_filter.hip) --------------------------------------------------------- *
 * Which events of a raw stream (x, y, t) on a W x H sensor are scene signal.  Polarity plays no part.
 * Event e at pixel (x, y) and time t is SUPPORTED iff there is an event e' != e at an in-sensor pixel (x', y') with
 * max(|x - x'|, |y - y'|) <= 1 that is not hot and is not (x, y) itself unless include_self, with 0 <= t - t' <= dt: ties count
 * (two neighbours with one timestamp support each other), t - t' = dt counts, dt + 1 does not.  keep(e) = (the pixel of e is
 * not hot) and supported(e).  The definition names no stream order: keep is a function of the multiset of events and repeats
 * bit for bit.
 * ren_event_support: pix_sorted (N int32 keys y * W + x in stable by-pixel order) and order (N int64, the stream index of each
 * sorted slot, a permutation of 0 .. N - 1) as for "event table"; ts_sorted (N int64): the timestamps IN THE SORTED ORDER,
 * non-decreasing inside every pixel's segment (they are when the stream is time-ordered: the CALLER checks that); seg
 * (H * W + 1 int32): seg[p] = the first sorted slot of pixel p, seg[H * W] = N; hot (H * W uint8, != 0 = hot; NULL = no pixel
 * is hot); dt >= 0, or dt < 0 for "every event is supported" (keep = not hot); include_self 0 or 1.  keep (N uint8, STREAM
 * order): keep[order[i]] for every sorted slot i, each stream index written exactly once.  One launch, one slot per lane per
 * trip of a grid-stride loop; per neighbour pixel a binary search of its segment for the last t' <= t.  Time differences are
 * signed 64-bit.  An order entry outside [0, N) is skipped (nothing read or written); a key outside [0, H * W) is not kept; segment
 * bounds are clamped to [0, N] before use.  No LDS, no atomics, no workgroup waits on another.
 * REN_ERR_BAD_ARG before any launch for a null or misaligned required pointer, N < 0, H or W < 1, include_self other than 0 / 1;
 * REN_ERR_UNSUPPORTED for N or H * W >= 2^31; N == 0 launches nothing. */
#define REN_EVENT_FILTER_THREADS 256         /* workgroup size */
#define REN_EVENT_FILTER_MAX_BLOCKS 2048     /* at most this many workgroups; the grid-stride loop takes the rest */
int ren_event_support(const int32_t *pix_sorted, const int64_t *order, const int64_t *ts_sorted, const int32_t *seg,
                      const uint8_t *hot, int64_t N, int32_t H, int32_t W, int64_t dt, int32_t include_self, uint8_t *keep,
                      void *stream);

/* ---- mesh (csrc/ren_mesh.hip) ------------------------------------------------------------------------- *
 * Triangle mesh of the level set sigma = level of a regular lattice of densities, by marching tetrahedra.  Everything below is
 * fixed by the lattice, so the output is the same index for index on every run and can be restated on the CPU.
 * Lattice: nx x ny x nz points (each >= 2, at most 2^30 in all) over the box [lo, hi]; point (i, j, k) at the linear index
 * (i * ny + j) * nz + k carries a float32 sigma and is INSIDE when sigma >= level (NaN outside, +inf inside, -inf outside).
 * Tetrahedra: every cube is cut into the six tetrahedra of the Freudenthal / Kuhn split, v0 = base, v1 = v0 + e_a, v2 = v1 + e_b,
 * v3 = v2 + e_c for the permutations (a, b, c) of the axes in lexicographic order (tetrahedron number 0 .. 5); they share the
 * body diagonal, and the split is the same in every cube, so neighbours agree on their face diagonals.
 * Edges: every tetrahedron edge leaves a lattice point p in one of seven directions e = 0 .. 6: (1,0,0), (0,1,0), (0,0,1),
 * (1,1,0), (1,0,1), (0,1,1), (1,1,1); p OWNS (p, e).  An edge whose far end lies outside the lattice does not exist.
 * Vertices: one on every existing edge whose ends differ in inside / outside, computed by the owner in float32, every operation
 * rounded on its own:  t = (level - sigma_p) / (sigma_q - sigma_p), replaced by 0.5 when not finite;
 * u = (float(i) + t di, float(j) + t dj, float(k) + t dk);  x = min(lo + u h, hi) per axis, h = (hi - lo) / (n - 1) computed by
 * the caller in float64 and passed as float32 (the min: the rounding of h can carry the last lattice plane an ulp past hi).
 * Vertex order: ascending lattice index, then e: id(p, e) = voff[p] + popcount(mask[p] & ((1 << e) - 1)), mask[p] = the 7-bit set
 * of crossed edges p owns, voff = the exclusive prefix sum of popcount(mask).
 * Triangles of a tetrahedron, corners named by its edges: one inside vertex a -> the edges to the three outside vertices in
 * ascending order of (v0 .. v3); three inside -> the edges from the outside vertex likewise; two inside a < b and two outside
 * c < d -> (ac, ad, bd) and (ac, bd, bc).  Orientation is COMBINATORIAL: the last two corners are swapped where the listed order
 * would point from the outside vertices to the inside ones, decided from the inside set and the parity of (a, b, c), never from
 * the computed positions; the normal points along -grad sigma.  Triangles of zero area (sigma == level at lattice points) are
 * kept and pair with their neighbours.  Face order: ascending cube index (i * (ny-1) + j) * (nz-1) + k, then tetrahedron, then
 * triangle.
 * ren_mesh_classify: sigma (nx*ny*nz float32) -> mask (uint8 per point), vcount (int32 per point, popcount of mask), fcount
 * (int32 per CUBE, (nx-1)(ny-1)(nz-1) entries at the cube index: 0 .. 12 triangles).  One launch.
 * ren_mesh_write: with voff / foff the exclusive prefix sums (int64, ren_exclusive_scan) of vcount / fcount and V / F their
 * totals: verts (V, 3) float32 and faces (F, 3) int32.  lo, hi, h: 3 floats each on the HOST.  One launch; a row at or beyond V
 * / F is not written.  V == 0 and F == 0 launches nothing.  No LDS, no atomics, no stack memory.
 * REN_ERR_BAD_ARG before any launch for an extent below 2, more than 2^30 points, a NaN level, a null or misaligned pointer
 * (verts / faces may be null when V / F is 0), V >= 2^31, V or F < 0, lo >= hi or h <= 0 on an axis, a box that is not finite. */
#define REN_MESH_THREADS 256                 /* workgroup size of both kernels: one lattice point per lane */
#define REN_MESH_MAX_POINTS (1 << 30)
int ren_mesh_classify(const float *sigma, int32_t nx, int32_t ny, int32_t nz, float level, uint8_t *mask, int32_t *vcount,
                      int32_t *fcount, void *stream);
int ren_mesh_write(const float *sigma, const uint8_t *mask, const int64_t *voff, const int64_t *foff, int32_t nx, int32_t ny,
                   int32_t nz, float level, const float *lo, const float *hi, const float *h, int64_t V, int64_t F, float *verts,
                   int32_t *faces, void *stream);

/* ---- mesh components (csrc/ren_mesh_components.hip) ---------------------------------------------------- *
 * Connected components of the lattice of "mesh": its solids (floaters among them) and, with outside != 0, its voids (cavities
 * among them).  Lattice, linear index p = (i * ny + j) * nz + k and INSIDE (sigma >= level; NaN outside) as in "mesh".
 * Selected set S: the inside points; with outside != 0 the complement, NaN points included.
 * Neighbours of p: p + e and p - e for the seven directions e of "mesh", (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1),
 * (1,1,1), where that point lies in the lattice: the ends of the marching-tetrahedra edges at p.  The other six diagonal pairs of
 * the 26-neighbourhood, (1,-1,0) for one, are NOT neighbours.  The same neighbourhood holds for S and for its complement: both
 * sides of the surface are connected along tetrahedron edges.
 * Component: an equivalence class of S under "joined by a chain of neighbours in S".
 * label[p] (int32, n = nx*ny*nz entries) = the smallest linear index of p's component, -1 for p not in S;
 * size[r] (int32, n entries) = the number of points of the component whose smallest index is r, 0 where r is no such root;
 * border[r] (uint8, n entries) = 1 when that component has a point on a face of the lattice (i in {0, nx-1}, or j, or k
 * likewise), else 0; 0 where r is no root.
 * All three are functions of (sigma, level, outside) alone: the result repeats bit for bit.
 * ren_mesh_components: three launches whatever the data (init; union by compare-and-swap of the larger root under the smaller,
 * every access to label a relaxed atomic of agent scope; flatten + count), no host read, no scratch beyond the outputs: label is
 * the parent array, size and border are cleared by the call.  No loop waits for another wave or workgroup.
 * ren_mesh_component_apply: one launch; out[p] = value where label[p] >= 0 and drop[label[p]] != 0 (drop: n uint8, indexed by
 * root), else the 32 bits of sigma[p] unchanged (NaN payloads survive).  out may alias sigma.  A label that is no index of the
 * n points drops nothing.  n == 0 launches nothing.
 * REN_ERR_BAD_ARG before any launch for an extent below 2, more than REN_MESH_MAX_POINTS points, a NaN level, a null pointer or
 * one not aligned to its element, n < 0, outside other than 0 or 1, a NaN value. */
int ren_mesh_components(const float *sigma, int32_t nx, int32_t ny, int32_t nz, float level, int32_t outside, int32_t *label,
                        int32_t *size, uint8_t *border, void *stream);
int ren_mesh_component_apply(const float *sigma, const int32_t *label, const uint8_t *drop, int64_t n, float value, float *out,
                             void *stream);

/* ---- mesh simplify (csrc/ren_mesh_simplify.hip) -------------------------------------------------------- *
 * Simplification of a triangle list by vertex clustering (Rossignac - Borrel): one vertex per occupied cell of a regular grid.
 * Everything below is fixed by the input, so the output is the same bit for bit on every run and can be restated on the CPU.
 * Input: verts (V, 3) float32; faces (F, 3) int32, ANY triangle list; a world box lo < hi (finite doubles on the HOST); a
 * cluster grid g = (gx, gy, gz), each >= 1, gx gy gz <= REN_MESH_MAX_POINTS; V and F below 2^31.
 * All real arithmetic is float64, every operation rounded on its own, with inv_a = g_a / (hi_a - lo_a) and
 * cw_a = (hi_a - lo_a) / g_a formed once on the host.
 * Cell of a vertex, per axis: r = (double(x_a) - lo_a) * inv_a, fl = floor(r); c_a = 0 if not fl >= 0 (NaN lands here), g_a - 1
 * if fl >= g_a, else int(fl).  Cell id (c_x * gy + c_y) * gz + c_z.  A vertex outside the box is clamped into the border cells;
 * nothing is refused for its position.
 * Representative: frac = r - double(c_a), 0 if not frac >= 0, 1 if frac > 1; q = uint64(floor(frac * 1048576.0 + 0.5)), in
 * [0, 2^20].  Per cell the three sums of q (uint64, below 2^51) and the member count (uint32) are accumulated with INTEGER
 * atomic adds: order-independent.  Position of the cell's vertex, per axis:
 *     float32(lo_a + (double(c_a) + double(sum_a) / double(count) / 1048576.0) * cw_a)
 * Provisional ids: the occupied cells in ascending cell id; id = coff[cell], coff the exclusive prefix sum (int64,
 * ren_exclusive_scan) of the occupied flags, `clusters` its total.
 * Faces: every corner is replaced by its cell's provisional id.  A face is DEGENERATE, and dropped, when a corner index is
 * outside [0, V) or two of its three ids are equal; the corner is range-checked before anything is read through it.  The KEY of
 * another face is its id triple rotated so that the smallest id comes first -- a rotation keeps the orientation: (A, B, C) and
 * (A, C, B) have different keys and both stay.  Among faces of equal key the one with the smallest input index survives, the
 * others are DUPLICATES.  Kept faces stay in input order and keep their own corner order, not the rotated one.
 * Orphans: a provisional vertex that no kept face references is removed; the others are renumbered in order (final id =
 * uoff[provisional id], the exclusive prefix sum of the used flags) and the faces follow.
 * Duplicates are found by ORDER, one method for every size: ren_mesh_simplify_faces writes the key as key_a = smallest id (int32)
 * and key_b = second << 31 | third (int64), INT32_MAX / INT64_MAX for a degenerate face; the caller orders the faces by (key_a,
 * key_b) with STABLE sorts (`order`: the input index at each sorted position), so that equal keys are adjacent in ascending
 * input index and the first of a run is its survivor.
 * ren_mesh_simplify_cells: cell[v] (int32), and sums (3 uint64 per cell) / count (uint32 per cell) += the members; the caller
 *   zeroes sums and count.  One launch, one vertex per lane; V == 0 launches nothing.
 * ren_mesh_simplify_flags: flag[c] (int32) = count[c] != 0.  One launch, one cell per lane.
 * ren_mesh_simplify_faces: ids (F, 3) int32 provisional ids ((-1, -1, -1) for a degenerate face), key_a, key_b, and
 *   *degenerate (int32, zeroed by the caller) += the number of degenerate faces.  One launch, one face per lane; F == 0 none.
 * ren_mesh_simplify_heads: keep[f] (int32) = 1 for the survivors, else 0; used[id] (int32, `clusters` entries zeroed by the
 *   caller) = 1 for every provisional id a survivor references.  One launch, one sorted position per lane; F == 0 none.
 * ren_mesh_simplify_vertices: the representative of every used cluster at row uoff[id] of verts (V_out, 3) float32, V_out the
 *   total of the used flags.  One launch, one cell per lane; V_out == 0 launches nothing.
 * ren_mesh_simplify_compact_faces: faces (F_out, 3) int32, row foff[f] (the exclusive prefix sum of keep, F_out its total) =
 *   uoff[ids[f]] per corner for the kept faces.  One launch, one face per lane; F_out == 0 launches nothing.
 * Every index read from memory (cell, coff, order, ids, foff, uoff) is compared with the extent of what it indexes before use.
 * Dense device memory: 28 B per cell for sums and count, 12 B more for the flag and its prefix sum; 30 GB + 13 GB at the cap.
 * REN_ERR_BAD_ARG before any launch for a null or misaligned pointer (one that a zero count leaves unused may be null), a grid
 * extent below 1, more than REN_MESH_MAX_POINTS cells, a count that is negative or 2^31 and beyond, clusters above the cells, V_out
 * above clusters, F_out above F, a box that is not finite with lo < hi. */
int ren_mesh_simplify_cells(const float *verts, int64_t V, const double *lo, const double *hi, int32_t gx, int32_t gy, int32_t gz,
                            int32_t *cell, uint64_t *sums, uint32_t *count, void *stream);
int ren_mesh_simplify_flags(const uint32_t *count, int64_t n_cells, int32_t *flag, void *stream);
int ren_mesh_simplify_faces(const int32_t *faces, int64_t F, int64_t V, const int32_t *cell, const int64_t *coff, int64_t n_cells,
                            int64_t clusters, int32_t *ids, int32_t *key_a, int64_t *key_b, int32_t *degenerate, void *stream);
int ren_mesh_simplify_heads(const int64_t *order, const int32_t *key_a, const int64_t *key_b, const int32_t *ids, int64_t F,
                            int64_t clusters, int32_t *keep, int32_t *used, void *stream);
int ren_mesh_simplify_vertices(const uint64_t *sums, const uint32_t *count, const int64_t *coff, const int32_t *used,
                               const int64_t *uoff, int32_t gx, int32_t gy, int32_t gz, const double *lo, const double *hi,
                               int64_t clusters, int64_t V_out, float *verts, void *stream);
int ren_mesh_simplify_compact_faces(const int32_t *ids, const int32_t *keep, const int64_t *foff, const int64_t *uoff, int64_t F,
                                    int64_t clusters, int64_t F_out, int32_t *faces, void *stream);

/* ---- mesh distance (csrc/ren_mesh_distance.hip) -------------------------------------------------------- *
 * Exact nearest neighbour of nq query points among nr reference points (both (n, 3) float32, counts below 2^31) through a
 * uniform grid of cubic cells: what surface-to-surface distances (accuracy, completeness, Chamfer, F-score) are made of.
 * Distance, float32, every operation rounded on its own: dx = q.x - p.x, dy, dz likewise; d2 = (dx*dx + dy*dy) + dz*dz.
 * Result per query: the minimum of d2 over the references and, among references of equal d2, the smallest index.  Both are
 * functions of the two point sets alone: they do not depend on lo, h or the grid, which only decide the work.
 * Grid: cells of edge h (inv_h its float32 reciprocal, |h * inv_h - 1| <= 2^-16) from the corner lo (three finite floats on
 * the HOST), g = (gx, gy, gz) cells, each extent in [1, REN_NN_MAX_EXTENT].  Cell of a point, per axis and in float32:
 * fl = floor((x_a - lo_a) * inv_h); c_a = 0 if not fl >= 0 (NaN lands here), g_a - 1 if fl >= g_a, else int(fl): a point
 * outside the box belongs to the nearest border cell.  Cell id (c_z * gy + c_y) * gx + c_x: x runs fastest.
 * ren_nn_cells: cell[i] (int32) of pts (n, 3).  One launch, one point per lane; n == 0 launches nothing.
 *   pts, n: the points; lo, inv_h, gx, gy, gz: the grid; cell: n int32 out.
 * The caller groups the references by cell (a stable sort of the ids) and hands ren_nn_search
 *   ref_records (nr, 4) float32, 16-byte aligned: row j = (x, y, z, the 32 bits of the ORIGINAL index as they stand) of the
 *     reference at sorted position j;
 *   cell_start (gx gy gz + 1) int32: the records of cell c are [cell_start[c], cell_start[c + 1]).
 * ren_nn_search: d2[q] (float32) and idx[q] (int32, an original index) for queries (nq, 3).  One launch, one query per lane,
 * in the caller's order (lanes whose queries share cells walk the same records: sort the queries by cell first).  From the
 * query's own cell (clamped as above) the lane visits the cells at Chebyshev distance r = 0, 1, 2, ..., clipped to the grid;
 * after shell r >= 1 it stops when best d2 < b * b with b = (float(r) - 2^-6) * h in float32, and after any shell when the
 * visited block covers the grid.  No reference outside the visited block can then have a d2 below or equal to the best one
 * (DESIGN 3.14), also for queries and references outside the box.  At most max(gx, gy, gz) shells; every range end read from
 * cell_start is clamped into [0, nr] before a record is read.  nr == 0 gives d2 = +inf, idx = -1; nq == 0 launches nothing.
 *   queries, nq; ref_records, cell_start, nr; lo, h, inv_h, gx, gy, gz: the grid the records were grouped on; d2, idx: nq out.
 * REN_ERR_BAD_ARG before any launch for a negative count or one of 2^31 and beyond, a grid extent below 1 or above
 * REN_NN_MAX_EXTENT, h or inv_h not positive and finite (h below FLT_MIN), h * inv_h further than 2^-16 from 1, lo null or
 * not finite, a null pointer that a positive count needs, a pointer not aligned to its element (ref_records: 16 bytes). */
#define REN_NN_MAX_EXTENT 512
int ren_nn_cells(const float *pts, int64_t n, const float *lo, float inv_h, int32_t gx, int32_t gy, int32_t gz, int32_t *cell,
                 void *stream);
int ren_nn_search(const float *queries, int64_t nq, const float *ref_records, const int32_t *cell_start, int64_t nr,
                  const float *lo, float h, float inv_h, int32_t gx, int32_t gy, int32_t gz, float *d2, int32_t *idx, void *stream);

/* ---- tsdf (csrc/ren_tsdf.hip) -------------------------------------------------------------------------- *
 * Fusion of posed z-depth maps into a truncated signed distance lattice: what a mesh of the RENDERED surface is extracted from.
 * Lattice nx x ny x nz, linear index p = (i * ny + j) * nz + k as in "mesh"; per point sum[p] (float32) and count[p] (int32),
 * READ AND UPDATED: the caller zeroes both before the first call, and a further call with further views continues the same
 * sums.  The views run in ascending order and every point adds its terms in that order, so the result does not depend on how
 * a sequence of views is split into calls, and it repeats bit for bit.
 *   depth (V, H, W) float32, device: z-depth along the optical axis; +inf = the ray met nothing, NaN or <= 0 = no information.
 *   cams (V, 12) float32, device: per view the centre c[3], then the camera-to-world rotation R[9] row-major (pos / rot of
 *     ren_raygen_fwd: column a of R is camera axis a, axis 2 looks forward).
 *   K5: five floats on the HOST, k00, k01, k02, k11, k12 of the upper-triangular pinhole matrix.
 *   lo, step: three float64 each on the HOST; step_a = (hi_a - lo_a) / (n_a - 1), formed by the caller in float64.
 * Per point and view, float32, every operation rounded on its own (no FMA), IEEE division:
 *   1. x_a = float32(lo_a + double(idx_a) * step_a): float64, the product and the sum rounded once each, then one rounding
 *   2. d_a = x_a - c_a
 *   3. q_a = (R[0][a] * d_0 + R[1][a] * d_1) + R[2][a] * d_2
 *   4. z = q_2; the view is skipped unless z > z_min (NaN skips)
 *   5. xn = q_0 / z, yn = q_1 / z
 *   6. u = (k00 * xn + k01 * yn) + k02, v = k11 * yn + k12
 *   7. fu = floorf(u + 0.5f), fv = floorf(v + 0.5f); skipped unless 0 <= fu < W and 0 <= fv < H (NaN skips): the nearest pixel,
 *      pixel (x, y) at the integer coordinates (x, y)
 *   8. D = depth[view][int(fv)][int(fu)]; skipped if D is NaN or D <= 0
 *   9. s = D - z; skipped if s < -trunc: the point is hidden behind the surface this view saw
 *  10. t = (s >= trunc) ? 1.0f : s / trunc (+inf gives 1)
 *  11. sum[p] += t, count[p] += 1
 * One launch, one lattice point per lane; the 12 floats of REN_TSDF_VIEW_BATCH views at a time are staged in LDS per workgroup.
 * No atomics.  V == 0 (or H * W == 0: every view skips every point) launches nothing.
 * REN_ERR_BAD_ARG before any launch for V, H or W negative, H or W above REN_TSDF_MAX_IMAGE, V * H * W of 2^31 and beyond, a
 * lattice extent below 2 or more than REN_MESH_MAX_POINTS points, trunc or z_min not positive and finite, lo or step not
 * finite, a step that is not positive, a null pointer that a positive count needs (K5, lo, step, sum and count always; cams
 * with V > 0; depth with V * H * W > 0), a pointer not aligned to its element. */
#define REN_TSDF_VIEW_BATCH 16               /* views whose cameras one workgroup stages in LDS at a time */
#define REN_TSDF_MAX_IMAGE 16384             /* H and W at most: pixel coordinates are exact in float32 */
int ren_tsdf_integrate(const float *depth, int32_t V, int32_t H, int32_t W, const float *cams, const float *K5, const double *lo,
                       const double *step, int32_t nx, int32_t ny, int32_t nz, float trunc, float z_min, float *sum, int32_t *count,
                       void *stream);

/* ---- utilities ------------------------------------------------------------------------------------- */
/* out[c] = sum_r in[r*C + c]  (C <= 4); scratch512: 512 floats of device scratch (two-stage, deterministic) */
int ren_column_sum(const float *in, int64_t rows, int32_t C, float *out, float *scratch512, void *stream);
/* NeRF.render_bkgd as a softplus-parametrised parameter (models/nerf.py:81-88): bkgd[C] = softplus(raw[C]); and its gradient
 * from the per-ray d_bkgd of ren_composite_bwd: grad_raw[c] += sigmoid(raw[c]) * sum_r d_bkgd_per_ray[r, c] */
int ren_bkgd_param_fwd(const float *raw, int32_t C, float *bkgd, void *stream);
int ren_bkgd_param_grad(const float *d_bkgd_per_ray, int64_t rows, int32_t C, const float *raw, float *grad_raw,
                        float *scratch512, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* REN_AMD_H */
