/*
 * gdb_nerf_hip.h — C ABI of libgdbnerf_hip.so: the GDB-NeRF depth-guided bundle-sampling hot
 * path as HIP kernels for gfx950 (MI355X).
 *
 * The reference (KLMAV-CUC/GDB-NeRF) is pure Python; it has no FFI of its own.  Each entry
 * point below replaces one Python operator of the reference (file:line relative to the
 * reference root) or one of the two third-party CUDA ops that operator calls.  The
 * reference-side binding a maintainer would add is a ctypes stub — see INTEGRATION.md.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch types.
 *  - Every pointer named d_* is DEVICE memory owned by the caller; the library never
 *    allocates, frees or retains device memory.  h_* pointers are host memory.
 *  - All tensors are contiguous float32 in the reference's own layouts unless stated.
 *  - Every function only ENQUEUES work on `stream` (a hipStream_t passed as void*); nothing
 *    synchronises with the host.  Data-dependent sample counts stay on the device.
 *  - Return value: GDB_OK (0) or a negative GdbStatus; gdb_last_error() returns a
 *    thread-local message for the last failure on the calling thread.  Shape / config
 *    violations are rejected before any launch.  The operator mirrors are NaN-transparent
 *    like the reference; the fused kernel at GDB_PREC_F16 converts activations to f16
 *    (|x| > 65504 becomes inf); at GDB_PREC_F32 it computes the MLP in fp32 throughout.
 *  - No process-global mutable state: every function is reentrant; the only per-thread state
 *    is the gdb_last_error() message.
 */
#ifndef GDB_NERF_HIP_H
#define GDB_NERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* v7 grew additively after its release: entries marked "(ABI v7, added)" are new functions, no existing signature or layout changed. */
#define GDB_ABI_VERSION 7

typedef enum GdbStatus {
    GDB_OK = 0,
    GDB_E_BADARG = -1,   /* null pointer, non-positive size, unsupported option */
    GDB_E_SHAPE = -2,    /* sizes inconsistent with each other or with the config */
    GDB_E_HIP = -3,      /* a HIP runtime call failed (message carries hipGetErrorString) */
    GDB_E_WORKSPACE = -4 /* workspace too small */
} GdbStatus;

/* Knobs of the path; names follow the reference's YAML keys (configs/dtu_pretrain.yaml:17-42,
 * read at networks/gdb_nerf/network.py:29-47). */
typedef struct GdbConfig {
    int32_t bundle_size;      /* nerf.bundle_size: b, power of two, 1..4 */
    int32_t max_num_samples;  /* nerf.max_num_samples: S_max, 1..GDB_MAX_SAMPLES */
    int32_t is_adaptive;      /* nerf.is_adaptive */
    int32_t inv_depth;        /* mvs.inv_depth[-1] */
    int32_t global_num_depth; /* nerf.global_num_depth */
    int32_t max_mipmap_level; /* nerf.max_mipmap_level, 0..GDB_MAX_MIP */
    int32_t feat_dim;         /* fpn.feat_dims[feat_level]: C_f (img_feat carries C_f+3 channels) */
    int32_t voxel_dim;        /* mvs.voxel_dim: C_v */
    int32_t hid_dim;          /* nerf.nerf_hidden_dims */
    int32_t viewdir_agg;      /* nerf.viewdir_agg */
} GdbConfig;

#define GDB_MAX_SAMPLES 16
#define GDB_MAX_MIP 3
#define GDB_MAX_VIEWS 8

/* One batch of hot-path inputs (Network.forward, network.py:114-166). */
typedef struct GdbFrame {
    int32_t B, V;             /* batch, source views */
    int32_t Ho, Wo;           /* target / source image size */
    int32_t H, W;             /* bundle map size: Ho/b, Wo/b */
    int32_t D;                /* depth planes of feat_volume */
    const float* d_src_images;  /* (B,V,3,Ho,Wo) */
    const float* d_img_feat;    /* (B,V,C_f+3,H,W): FPN level ⊕ downsampled RGB, network.py:159-164 */
    const float* d_feat_volume; /* (B,C_v,D,H,W) */
    const float* d_depth_range; /* (B,2,H,W) near/far of the depth prior */
    const float* d_vol_range;   /* (B,2,H,W) near/far of the cost volume */
    const float* d_src_exts;    /* (B,V,4,4) world-to-camera */
    const float* d_src_ints;    /* (B,V,3,3) */
    const float* d_tar_exts;    /* (B,4,4) world-to-camera */
    const float* d_tar_ints;    /* (B,3,3) */
    const float* d_near_far;    /* (B,2) scene near/far */
} GdbFrame;

/* ---- library ------------------------------------------------------------------------ */
int gdb_abi_version(void);
const char* gdb_last_error(void);

/* Bytes of device workspace gdb_prepare() needs for a frame of this shape (camera block,
 * channel-last feature pyramid, per-bundle counts/offsets). */
int gdb_workspace_bytes(const GdbConfig* cfg, const GdbFrame* shape, size_t* out_bytes);

/* Where gdb_prepare() puts the feature pyramid inside the workspace, for callers that want to read it
 * back (it is what nvdiffrast builds inside texture(): bundle_sampler.py:355-359).  Per (batch, view) the
 * pyramid is [level][chunk 0..4][y][x] of 16-byte texel chunks (channels 4*chunk .. 4*chunk+3 of the
 * C_f+3 = 19 channels, channel 19 zero).  out[0] = byte offset of the first pyramid, out[1] = floats per
 * (batch, view) pyramid, out[2] = number of mip levels built beyond level 0 (stops at the first level with
 * an odd extent), out[3 + l] = float offset of level l inside one pyramid, l = 0..3. */
int gdb_pyramid_layout(const GdbConfig* cfg, const GdbFrame* shape, size_t out[7]);

/* Where the plan of the dense schedule (GDB_SCHED_DENSE) lives, for callers / tests that want to read it: per bundle-map row
 * (B*H rows) out[1] int32 values [n_windows, first sample offset of window 0 .. n_windows-1, the row's sample total].  A window
 * is a run of WHOLE consecutive bundles holding at most 32 samples (offsets = exclusive prefix of the per-bundle sample counts
 * along the row, bundle_sampler.py:179-189) - one wave of the dense kernel, lane = sample.  Rows of 1024 .. 4095 sample offsets
 * (W * S_max) are cut greedily (a window ends only where the next bundle would not fit); shorter and longer rows at fixed offsets: window w =
 * the bundles whose first sample offset falls into [out[2] * w, out[2] * (w + 1)), out[2] = 33 - S_max.  out[0] = byte offset of
 * the first row record.  Built by gdb_prepare FROM THE CONTENTS OF d_depth_range AT THAT TIME when the frame carries it and the
 * config is adaptive; a dense render that is not told the plan is current (GDB_SCHED_PLAN_READY) rebuilds it first. */
int gdb_dense_plan_layout(const GdbConfig* cfg, const GdbFrame* shape, size_t out[3]);
/* ... and the compacted sample list beside it (bundle_sampler.py:182-189: bundle-major, sample-minor): per bundle-map row out[1]
 * uint32 entries, entry s = the sample at offset s of the row as [bundle x | slot k << 16 | count of the bundle << 24],
 * 0xFFFFFFFF past the row's last sample.  out[0] = byte offset of the first row.  Window w of the plan is the wave that reads
 * the entries [start_w, start_{w+1}) of its row. */
int gdb_dense_map_layout(const GdbConfig* cfg, const GdbFrame* shape, size_t out[2]);

/* ---- MLP weights -------------------------------------------------------------------- */
/* Number of floats in the packed weight buffer for cfg (fp32 section + MFMA-fragment
 * section). */
int gdb_packed_weight_floats(const GdbConfig* cfg, size_t* out_floats);
/* Pack the 18 NeRF tensors (state-dict order of networks/gdb_nerf/nerf.py:20-56:
 * view_fc.0, global_fc.0, agg_w_fc.0, fc.0, lr0.0, sigma.0, weight.0, weight.2,
 * feat_head.0; each .weight (out,in) row-major then .bias) into h_out.  Host only; the
 * caller uploads h_out to the device once per checkpoint.  If viewdir_agg is 0 the first
 * two pointers may be NULL. */
int gdb_pack_weights(const GdbConfig* cfg, const float* const h_tensors[18], float* h_out);

/* ---- per-frame preparation ---------------------------------------------------------- */
/* Camera block (matrix inverses, ray matrix, pixel radii: bundle_sampler.py:67-74,304-313)
 * and the channel-last mip pyramid of img_feat (what nvdiffrast.texture builds on every
 * call, bundle_sampler.py:355-359).  d_tar_exts, d_tar_ints, d_near_far are required; the source
 * side (d_src_exts + d_src_ints, d_img_feat) may be NULL when only gdb_build_rays / gdb_sample follow.
 * The workspace also reserves room for the per-bundle
 * sample counts and their exclusive scan, which gdb_sample fills
 * (bundle_sampler.py:179,182-189).
 * What gdb_prepare READS: the camera matrices, d_near_far, d_img_feat (and d_src_images in the _fpn form) - and, when the frame
 * carries d_depth_range and the config is adaptive, THE CONTENTS OF d_depth_range AS THEY ARE AT THIS CALL, from which it builds
 * the dense schedule's per-row plan and compacted sample list (gdb_dense_plan_layout / gdb_dense_map_layout).  A render call
 * uses that plan only when told it is current (GDB_SCHED_PLAN_READY); otherwise it rebuilds it from the frame it is given. */
int gdb_prepare(const GdbConfig* cfg, const GdbFrame* frame, void* d_workspace, size_t workspace_bytes,
                void* stream);

/* The same from the FPN output (next row N3): d_fpn_feat (B,V,C_f,H,W) is the feature level alone; the three colour
 * channels the reference concatenates (network.py:159-164: F.interpolate(src_images, size=(H,W), mode='bilinear',
 * align_corners=False)) are resampled from frame->d_src_images inside the same launch.  frame->d_img_feat is ignored. */
int gdb_prepare_fpn(const GdbConfig* cfg, const GdbFrame* frame, const float* d_fpn_feat, void* d_workspace,
                    size_t workspace_bytes, void* stream);

/* ---- operator mirrors (one per reference method) ------------------------------------ */
/* gdb_prepare / gdb_prepare_fpn (d_fpn_feat may be NULL: the gdb_prepare form) with options.  ABI v5.
 *   GDB_PREP_PYR16  also write the HALF-PRECISION copy of the feature pyramid, in the same launch, from the same registers: what a
 *                   GDB_PREC_F16 render gathers its feature taps from (16 + 4 bytes per tap and lane instead of 16 + 16 + 8, two
 *                   load instructions instead of three; values = the fp32 pyramid's, rounded to nearest half once, every mip level
 *                   box-filtered in fp32 first).  Replaces nothing of the reference: nvdiffrast rebuilds its fp32 mip stack inside
 *                   every texture() call (bundle_sampler.py:355-359); this is a second, narrower copy for the opt-in fast path.
 *                   Pass GDB_SCHED_PYR16_READY to the render calls of this frame.
 *   GDB_PREP_PYR16_ONLY  (with GDB_PREP_PYR16) write ONLY the half-precision pyramid: the fp32 pyramid in the workspace is left as
 *                   it was (26 of the 58 MB k_prepare moves at 512x640, V = 3).  Only GDB_PREC_F16 fused renders may follow; gdb_encode, the
 *                   f32 / split-f16 renders and gdb_build_pyr16 read the fp32 pyramid and need a prepare without this flag first
 *                   (like GDB_SCHED_PLAN_READY this is the caller's promise: the library keeps no state to check it against).
 *   (GDB_PREP_PYR16, in full: besides the pyramid it writes a HALF-PRECISION RGBA COPY OF frame->d_src_images behind it - 8 bytes per
 *                   pixel, halves (r, g, b, 0) - from which the GDB_PREC_F16 kernels read their colour taps (one 16-byte load per x pair of a
 *                   tap row).  So with this flag the colours a later f16 render sees are those of d_src_images AT THIS CALL:
 *                   GDB_SCHED_PYR16_READY is the promise that neither d_img_feat / d_fpn_feat nor d_src_images have changed since.
 *                   A frame that carries a feature map but no d_src_images is refused with this flag (GDB_E_BADARG).  The copy is made
 *                   for bundle_size 2 (the fused kernels' size) only; gdb_pyramid16_layout does not describe it: it starts at the
 *                   first 256-byte boundary behind the B * V pyramid blocks + 16 bytes of padding.)
 *   GDB_PREP_SOURCES_READY  (ABI v7) the caller vouches that everything in the workspace that depends on the SOURCE views alone - the fp32
 *                   pyramid, and with GDB_PREP_PYR16 the half-precision pyramid and image copy - was built by an earlier gdb_prepare*
 *                   call on this workspace, with the same flags, from d_img_feat / d_fpn_feat / d_src_images whose contents have not
 *                   changed: this call rebuilds the camera block (target AND source records) and the list schedules' plan only - what
 *                   a sweep of target views over fixed source views needs per view (bundle_sampler.py:304-313 recomputes the camera
 *                   terms per call; nvdiffrast rebuilds the mip stack per call, :355-359 - this flag is where this library does not).
 *                   Like the two render-side promises the library keeps no state to check it against. */
#define GDB_PREP_PYR16 1
#define GDB_PREP_PYR16_ONLY 2
#define GDB_PREP_SOURCES_READY 4
/* gdb_prepare_rows only: whether a strip smaller than the frame builds just its reach of the source-only products (see there).  Neither
 * flag: by size - the bound costs a launch of its own ahead of the tiles (~8 us of stream time), which pays once the whole-frame tile
 * work moves >= 128 MB (1200x1600 with 5 views at f16: 95 -> 46 us per rank at 8 ranks; at 512x640 it would cost 3 us more than it saves:
 * profiles/r06/time_prepare_rows_world8.json). */
#define GDB_PREP_STRIP_REACH 8   /* always build the strip's reach only */
#define GDB_PREP_STRIP_WHOLE 16  /* always build the whole pyramid (a later render of other rows stays valid) */
#define GDB_PREP_ALL (GDB_PREP_PYR16 | GDB_PREP_PYR16_ONLY | GDB_PREP_SOURCES_READY | GDB_PREP_STRIP_REACH | GDB_PREP_STRIP_WHOLE)
int gdb_prepare_ex(const GdbConfig* cfg, const GdbFrame* frame, const float* d_fpn_feat, int32_t flags, void* d_workspace,
                   size_t workspace_bytes, void* stream);

/* gdb_prepare_ex for a rank that renders ONE row strip of the frame (multi-GPU row sharding; ABI v6): the camera block as
 * ever, the list schedules' plan for the bundle-map rows [row_begin, row_end) of every batch item only - the rows outside the strip are
 * another rank's - and, when the strip is smaller than the frame (round 6), only the PART of the source-only products the strip's samples
 * can reach: per (batch, view) a launch of its own ahead of the tiles (k_strip_bounds) takes the extremes of the strip's depth prior
 * (a sample's depth lies between its bundle's near and far, bundle_sampler.py:122-191), projects the 8 vertices of the convex body
 * { o + d(x, y) z : (x, y) in the strip's pixel rectangle, z in [z_min, z_max] } (bundle_sampler.py:67-71, :254-256) into the view and
 * builds only the 32 x 8-texel pyramid tiles (all mip levels) and the image rows (half-precision copy) inside that box + the mip /
 * bilinear margins; a view it cannot bound (a vertex behind or near the camera plane, a non-finite or non-positive depth) is built
 * whole.  It reads d_depth_range, so the frame must carry it.  GDB_SCHED_PLAN_READY holds for render calls whose strip lies inside
 * [row_begin, row_end); RENDERS OF ROWS OUTSIDE IT ARE INVALID on this workspace until a prepare of the whole frame (and so are
 * gdb_encode / GDB_PREP_SOURCES_READY, which read the whole pyramid). */
int gdb_prepare_rows(const GdbConfig* cfg, const GdbFrame* frame, const float* d_fpn_feat, int32_t flags, int32_t row_begin,
                     int32_t row_end, void* d_workspace, size_t workspace_bytes, void* stream);

/* Where the half-precision pyramid sits in the workspace (tests / callers that read it): out[0] = byte offset, out[1] = bytes per
 * (batch, view), out[2] = mip levels beyond 0, out[3 + l] = byte offset of level l inside a (batch, view) block.  A level of hw
 * texels is three planes: [0, 16 hw) 16 bytes per texel = halves of channels 0..3, 8..11; [16 hw, 32 hw) channels 4..7, 12..15;
 * [32 hw, 40 hw) 8 bytes per texel = channels 16..19 (19 is padding). */
int gdb_pyramid16_layout(const GdbConfig* cfg, const GdbFrame* shape, size_t out[7]);

/* BundleSampler.build_rays, bundle_sampler.py:30-74.  Needs gdb_prepare on the same
 * workspace first.  Outputs: d_rays_d (B,Ho,Wo,3), d_uv (Ho,Wo,2), d_rays_o (B,3),
 * d_z_axis (B,3), d_tar_pixel_radius (B). */
int gdb_build_rays(const GdbConfig* cfg, const GdbFrame* frame, const void* d_workspace, float* d_rays_d,
                   float* d_uv, float* d_rays_o, float* d_z_axis, float* d_tar_pixel_radius, void* stream);

/* BundleSampler.sample, bundle_sampler.py:193-265.  Needs gdb_prepare first.  Arrays are
 * sized for the maximum N_max = B*H*W*S_max; the first *d_total entries are valid, in the
 * reference's order (bundle-major, sample-minor).  d_rays_xyz (N_max,3,b*b), d_uvd (N_max,3),
 * d_z_vals, d_ball_radii (N_max), d_indices int64 (N_max), d_samples_per_batch int64 (B),
 * d_samples_per_bundle int32 (B*H*W), d_total int64 (1). */
int gdb_sample(const GdbConfig* cfg, const GdbFrame* frame, void* d_workspace, float* d_rays_xyz,
               float* d_uvd, float* d_z_vals, float* d_ball_radii, int64_t* d_indices,
               int64_t* d_samples_per_batch, int32_t* d_samples_per_bundle, int64_t* d_total, void* stream);

/* BundleSampler.encode, bundle_sampler.py:267-371 (including the nvdiffrast.torch.texture
 * call at :355-359 and the two F.grid_sample calls at :323,:336).  Needs gdb_prepare first.
 * n_alloc = rows allocated in the sample arrays / outputs; the valid count is read on the
 * device from d_total and d_samples_per_batch.  Outputs d_rgbs_feat_dir (V,n_alloc,3b²+C_f+3+4),
 * d_vox_feat (n_alloc,C_v). */
int gdb_encode(const GdbConfig* cfg, const GdbFrame* frame, const void* d_workspace, const float* d_rays_xyz,
               const float* d_uvd, const float* d_ball_radii, const int64_t* d_samples_per_batch,
               const int64_t* d_total, int64_t n_alloc, float* d_rgbs_feat_dir, float* d_vox_feat,
               void* stream);

/* NeRF.forward, networks/gdb_nerf/nerf.py:84-115, exact fp32.  d_rgbs_feat_dir (V,n_alloc,P)
 * with P = 3b²+C_f+3+4; rows [0,n) are processed (n from *d_total when d_total != NULL, else
 * n_alloc).  Outputs d_sigma (n_alloc), d_feat (n_alloc, P-4+C_v). */
int gdb_mlp(const GdbConfig* cfg, const float* d_packed_weights, int32_t V, const float* d_vox_feat,
            const float* d_rgbs_feat_dir, const int64_t* d_total, int64_t n_alloc, float* d_sigma,
            float* d_feat, void* stream);

/* render_weight_from_density + accumulate_value_along_rays, networks/gdb_nerf/utils.py:19-43,
 * 88-121 (nerfacc.volrend.render_weight_from_alpha / accumulate_along_rays at :35,:110), with
 * the inv_depth handling of Network.render_bundles, network.py:83-89.  d_indices sorted
 * ascending.  channels = columns of d_feat.  Outputs d_weights (n_alloc), d_bundle_feat
 * (n_bundles,channels), d_depth, d_opacity (n_bundles). */
int gdb_composite(const GdbConfig* cfg, const float* d_sigma, const float* d_feat, const float* d_z_vals,
                  const int64_t* d_indices, const int64_t* d_total, int64_t n_alloc, int64_t n_bundles,
                  int32_t channels, float* d_weights, float* d_bundle_feat, float* d_depth, float* d_opacity,
                  void* d_scratch_2xnbundles_i32, void* stream);

/* render_weight_from_density alone, networks/gdb_nerf/utils.py:19-43 (alpha = 1-exp(-sigma);
 * nerfacc.volrend.render_weight_from_alpha :35; per-bundle normalisation :38-41).
 * d_scratch: 2*n_bundles int32. */
int gdb_render_weights(const GdbConfig* cfg, const float* d_sigma, const int64_t* d_indices, const int64_t* d_total,
                       int64_t n_alloc, int64_t n_bundles, float* d_weights, void* d_scratch_2xnbundles_i32, void* stream);

/* accumulate_value_along_rays alone, networks/gdb_nerf/utils.py:88-121
 * (nerfacc.volrend.accumulate_along_rays :110): segmented sum of weights * [feat | z | 1].  z_vals are
 * used as given (the caller applies inv_depth as Network.render_bundles does). */
int gdb_accumulate(const GdbConfig* cfg, const float* d_weights, const float* d_feat, const float* d_z_vals,
                   const int64_t* d_indices, const int64_t* d_total, int64_t n_alloc, int64_t n_bundles, int32_t channels,
                   float* d_feat_map, float* d_depth_map, float* d_opacity_map, void* d_scratch_2xnbundles_i32,
                   void* stream);

/* ---- backward of the operator mirrors (training) ----------------------- */
/* Gradients of gdb_mlp, gdb_render_weights and gdb_accumulate, fp32.  Nothing is saved between forward and backward: every
 * entry recomputes what it needs from the forward's inputs.  No floating-point atomics: results are bit-identical from run
 * to run.  gdb_encode has a backward with respect to the values it gathers (gdb_encode_backward below) and one with
 * respect to the sample positions (gdb_encode_position_backward), gdb_sample one with respect to the depth prior (gdb_sample_backward;
 * DESIGN.md 4.16); the fused entries and the decoder have none.
 *
 * gdb_mlp_backward_layout: out[0] = workspace bytes of gdb_mlp_backward, out[1] = partials (workgroups) per launch,
 * out[2] = samples per tile.  V < 2 is refused with GDB_E_SHAPE (the unbiased variance over views has no derivative there). */
int gdb_mlp_backward_layout(const GdbConfig* cfg, int32_t V, int64_t n_alloc, size_t out[3]);

/* d_g_sigma (n_alloc), d_g_feat (n_alloc, P-4+C_v): upstream gradients of gdb_mlp's outputs.  d_g_packed receives the gradient
 * of all 18 tensors in the layout of the packed fp32 section (its first floats; gdb_unpack_weight_grads takes it apart; pad
 * slots are zero, view_fc's slots are zero without viewdir_agg).  d_g_vox (n_alloc, C_v) and d_g_rgbs_feat_dir (V, n_alloc, P)
 * may be NULL.  Rows [*d_total, n_alloc) add nothing to the weight gradients and get zero rows in both. */
int gdb_mlp_backward(const GdbConfig* cfg, const float* d_packed_weights, int32_t V, const float* d_vox_feat,
                     const float* d_rgbs_feat_dir, const int64_t* d_total, int64_t n_alloc, const float* d_g_sigma,
                     const float* d_g_feat, float* d_g_packed, float* d_g_vox, float* d_g_rgbs_feat_dir, void* d_workspace,
                     size_t workspace_bytes, void* stream);

/* Host inverse of gdb_pack_weights' fp32 section: copies each tensor's gradient out of h_packed (order and sizes as
 * gdb_pack_weights; the two view_fc pointers are ignored without viewdir_agg). */
int gdb_unpack_weight_grads(const GdbConfig* cfg, const float* h_packed, float* const h_tensors[18]);

/* d_g_weights (n_alloc) -> d_g_sigma (n_alloc); samples of no bundle and rows past *d_total get 0.  The clamp of the weight
 * sum at 1e-6 has derivative 0 below it. */
int gdb_render_weights_backward(const GdbConfig* cfg, const float* d_sigma, const int64_t* d_indices, const int64_t* d_total,
                                int64_t n_alloc, int64_t n_bundles, const float* d_g_weights, float* d_g_sigma,
                                void* d_scratch_2xnbundles_i32, void* stream);

/* d_g_feat_map (n_bundles, channels), d_g_depth_map, d_g_opacity_map (n_bundles) -> d_g_weights (n_alloc), d_g_feat (n_alloc,
 * channels).  This entry gives d_z_vals no gradient: it is weights * g_depth_map[indices], which the Python AccumulateFunction forms
 * in torch when z_vals carries a graph.  d_scratch is not read by this version and may be NULL. */
int gdb_accumulate_backward(const GdbConfig* cfg, const float* d_weights, const float* d_feat, const float* d_z_vals,
                            const int64_t* d_indices, const int64_t* d_total, int64_t n_alloc, int64_t n_bundles, int32_t channels,
                            const float* d_g_feat_map, const float* d_g_depth_map, const float* d_g_opacity_map,
                            float* d_g_weights, float* d_g_feat, void* d_scratch_2xnbundles_i32, void* stream);

/* ---- backward of gdb_encode with respect to the gathered values (ABI v7, added) ---- */
/* With the sample positions held constant gdb_encode is linear in img_feat (through the 2x2 box mip chain and the
 * linear-mipmap-linear fetch) and in feat_volume (trilinear, border): the backward is the transpose of the gather, a scatter-add.
 * This entry gives no gradient to d_rays_xyz, d_uvd and d_ball_radii (gdb_encode_position_backward below does); the cameras and
 * d_src_images get none anywhere.
 *
 * Reproducible by fixed point, not by order: G = max |upstream| over the rows [0, *d_total) of d_g_vox and of the C_f + 3 feature
 * columns of d_g_rgbs_feat_dir (both, whichever outputs are asked for); with e = ceil(log2 G) every contribution w * g is formed in
 * double, scaled by 2^(F - e), rounded to a 64-bit integer and added with one integer atomic - integer addition is associative, so
 * two calls on the same inputs give bit-identical outputs.  F = min(40, 62 - ceil(log2(8 n_alloc))): one destination receives at
 * most 8 n_alloc contributions of magnitude <= 2^e (8 volume taps, or the 4 texture taps of one level when both axes clamp), so no
 * sum leaves int64.  Absolute resolution of a contribution: 2^(e - F).  G == 0: the outputs are exact zeros.  G not finite (an inf or
 * a NaN in a valid upstream row cannot be scaled): the requested outputs are filled with NaN.
 *
 * gdb_encode_backward_layout: out[0] = bytes of d_bwd_workspace, out[1] = F, out[2] / out[3] = byte offsets of the accumulators
 * inside it - pyramid: int64 [B * V][level][y][x][20] with the level offsets of gdb_pyramid_layout (in texels of 20), channel 19 unused;
 * volume: int64 [B][z][y][x][C_v].  n_alloc outside 1 .. B*H*W*S_max is GDB_E_SHAPE, out == NULL GDB_E_BADARG. */
int gdb_encode_backward_layout(const GdbConfig* cfg, const GdbFrame* shape, int64_t n_alloc, size_t out[4]);

/* d_workspace: the workspace gdb_prepare filled for THIS frame, read-only - its camera block and the level geometry are used, not
 * the pyramid's contents; the frame's device pointers are not read.  The sample arrays are those gdb_encode was given.
 * d_g_rgbs_feat_dir (V, n_alloc, P) and d_g_vox (n_alloc, C_v): upstream gradients of gdb_encode's outputs, both required.
 * d_g_img_feat (B, V, C_f+3, H, W) and d_g_feat_volume (B, C_v, D, H, W): either may be NULL, and then its scatter is not run; both
 * NULL is GDB_E_BADARG.  Rows [*d_total, n_alloc) contribute nothing, whatever they hold.  d_bwd_workspace is zeroed here. */
int gdb_encode_backward(const GdbConfig* cfg, const GdbFrame* frame, const void* d_workspace, const float* d_rays_xyz,
                        const float* d_uvd, const float* d_ball_radii, const int64_t* d_samples_per_batch, const int64_t* d_total,
                        int64_t n_alloc, const float* d_g_rgbs_feat_dir, const float* d_g_vox, float* d_g_img_feat,
                        float* d_g_feat_volume, void* d_bwd_workspace, size_t bwd_workspace_bytes, void* stream);

/* ---- backward of gdb_encode with respect to the sample positions, and of gdb_sample (ABI v7, added) ---- */
/* Derivative conventions of both entries (what torch autograd of the plain-torch restatement does):
 *  - tap indices, fractions, the mip level and every clamp decision are the forward's own bits (the forward's helpers, called in the
 *    same order under the same compile contract); the derivative arithmetic runs in double and is rounded to float once per output.
 *  - d/dx of a bilinear / trilinear fetch is (1 - f_y)(t01 - t00) + f_y (t11 - t10), times the coordinate scale: W_o / 2 for the
 *    sub-ray colours, W_l per mip level for the feature texture, D / 2 for the volume's depth axis.  A coordinate clamped by border /
 *    clamp-to-edge addressing has derivative 0, equality included (torch's grid_sample rule).
 *  - the mip level clamped to [0, L] passes its derivative inside the interval and 0 outside; a NaN level gives 0.  d out / d level is
 *    tex(l1) - tex(l0) where the blend fraction was used; both blended levels contribute to d / d(u, v) with their blend weights.
 *  - clamp_min floors (1e-6 on the two projected depths, 1e-12 under the two square roots of the mip level, 1e-12 in the ball radius
 *    per unit distance and in F.normalize): derivative 0 below the floor.
 *  - no floating-point atomics and no order that depends on arrival: two calls on the same inputs give bit-identical outputs.
 *
 * gdb_encode_position_backward.  d_workspace: the workspace gdb_prepare filled for THIS frame.  Unlike gdb_encode_backward this entry
 * reads the pyramid's contents, the frame's feature volume and its source images: the derivative of a bilinear fetch is a
 * difference of the fetched texels.  The sample arrays and the two upstream gradients are those of gdb_encode_backward.
 * Outputs d_g_rays_xyz (n_alloc, 3, b*b), d_g_uvd (n_alloc, 3), d_g_ball_radii (n_alloc): each may be NULL, all three NULL is
 * GDB_E_BADARG.  Rows [*d_total, n_alloc) of every output are written as zeros and are never read, whatever they hold.  n_alloc
 * outside 1 .. B*H*W*S_max is GDB_E_SHAPE.
 * Columns 0 and 1 of d_g_uvd are written as zeros and are NOT differentiated: u, v are the bundle's pixel centre, depend on no
 * trainable tensor and sit exactly on voxel centres, where the trilinear derivative is one-sided.  Column 2 is the gradient of the
 * normalised depth.  Per view: sub-ray point -> camera -> image -> the colour taps (3 b*b columns, each sub-ray its own path);
 * centre mean_s(E p_s) -> (u, v, level) -> the C_f + 3 feature columns (d_ball_radii enters through the level only); centre
 * mean_s p_s -> the four direction columns.  d_g_rays_xyz[i, :, s] is the sum of the three paths over the views v = 0 .. V-1 in
 * that order. */
int gdb_encode_position_backward(const GdbConfig* cfg, const GdbFrame* frame, const void* d_workspace, const float* d_rays_xyz,
                                 const float* d_uvd, const float* d_ball_radii, const int64_t* d_samples_per_batch,
                                 const int64_t* d_total, int64_t n_alloc, const float* d_g_rgbs_feat_dir, const float* d_g_vox,
                                 float* d_g_rays_xyz, float* d_g_uvd, float* d_g_ball_radii, void* stream);

/* gdb_sample_backward.  d_workspace: prepared for the frame gdb_sample ran on (its target camera; the frame's d_depth_range /
 * d_vol_range are read).  d_samples_per_bundle int32 (B*H*W): the counts gdb_sample returned - they are data: the derivative of
 * ceil / clamp is 0; the sample offsets come from the same exclusive scan of them.  Upstream gradients of gdb_sample's outputs,
 * n_alloc rows each, each may be NULL (= zero): d_g_rays_xyz (n_alloc, 3, b*b), d_g_uvd (n_alloc, 3; only column 2 is read),
 * d_g_z_vals, d_g_ball_radii (n_alloc); all four NULL is GDB_E_BADARG.  Outputs d_g_depth_range, d_g_vol_range (B, 2, H, W): either
 * may be NULL, both NULL is GDB_E_BADARG.  One bundle's four scalars receive the sum over its <= S_max samples in sample order; rows
 * [*d_total, n_alloc) are not read.  Chain: t_k = n + (f - n)(k + 1/2) / c in sampling space; d = 2 (t - v_n) / (v_f - v_n) - 1;
 * z = t, or 1 / t under inv_depth; rays_xyz = o + dir z; ball = unit |mean dir| |z|; under inv_depth the four ranges are inverted
 * first (-1 / x^2 on the way back).  d_scratch: 4 * (B*H*W + ceil(B*H*W / 1024)) bytes. */
int gdb_sample_backward(const GdbConfig* cfg, const GdbFrame* frame, const void* d_workspace, const int32_t* d_samples_per_bundle,
                        const int64_t* d_total, int64_t n_alloc, const float* d_g_rays_xyz, const float* d_g_uvd,
                        const float* d_g_z_vals, const float* d_g_ball_radii, float* d_g_depth_range, float* d_g_vol_range,
                        void* d_scratch, void* stream);

/* ---- production entry ---------------------------------------------------------------- */
/* The whole hot-path section of Network.forward (network.py:145-169: build_rays → sample →
 * encode → render_bundles) in one pass with no intermediate in HBM.  Needs gdb_prepare on
 * the same workspace first.  row_begin/row_end select a strip of bundle-map rows
 * [row_begin,row_end) of every batch item (multi-GPU row-strip sharding); outputs are full
 * size and only the strip's rows are written.
 *
 * precision (arithmetic of the NeRF MLP, nerf.py:84-115; fetch, geometry and composite are fp32 either way):
 *   GDB_PREC_F16  f16 MFMA operands, fp32 accumulate (v_mfma_f32_32x32x16_f16) — narrower than the reference;
 *   GDB_PREC_F32  fp32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fp32 fmaf chain, one rounding per product) —
 *                 the reference's own precision.
 *   GDB_PREC_F32X split-f16: every MFMA operand as an f16 pair hi + lo (about 22 bits), a product as lo·hi + hi·lo + hi·hi on
 *                 v_mfma_f32_32x32x16_f16 with fp32 accumulate — fp32-grade (not bit-exact fp32) at close to the f16 rate.
 *                 Like GDB_PREC_F16 it assumes activations inside the f16 range: the high half saturates at 65504 (the low
 *                 half then carries the rest up to about twice that; beyond it the value is clipped).  Operand range of the
 *                 "22 bits": the low half of a value below 2^-3 is an f16 subnormal (resolution 2^-24), so a pair carries an
 *                 ABSOLUTE error floor of 2^-25 per operand: |x| >= 0.125 keeps ~22 bits, |x| = 1e-3 about 15, and below 6e-5
 *                 the high half is subnormal too (plain f16 accuracy).  Measured on the MLP with every weight scaled (profiles/
 *                 r03/split_f16_small_operands.txt): |f32x - f32| / output scale 5e-7 at x1, 1.5e-6 at x0.2, 5e-6 at x0.05,
 *                 3e-5 at x0.01, 2e-4 (= GDB_PREC_F16's) at x0.001.  Weights are not rescaled at pack time: use GDB_PREC_F32 for
 *                 checkpoints with layers of such small magnitude.
 * schedule (work decomposition; results agree to rounding): GDB_SCHED_AUTO picks by shape, GDB_SCHED_SLOT_WAVES =
 *   one wave per sample slot with the composite through LDS, GDB_SCHED_SEGMENT_WAVE = one wave walks all slots of
 *   its 32 bundles with the composite in registers, GDB_SCHED_DENSE = the reference's compacted sample list
 *   (bundle_sampler.py:182-189): one wave per window of WHOLE consecutive bundles of a bundle-map row holding <= 32 samples,
 *   composite across lanes; GDB_SCHED_FLAT = the same list read as one list over the rows and cut into windows of EXACTLY 32
 *   consecutive samples (4-8 % fewer waves; a bundle may straddle two windows - both waves then leave its samples' records in
 *   d_workspace and whichever of the two arrives last at the boundary's counter composites it, inside the same launch, with the in-wave
 *   composite's own arithmetic, bit for bit: the result depends neither on where the windows fall nor on the order of arrival, row strips
 *   equal the full render; bit-identical to GDB_SCHED_DENSE.  The counters live in d_workspace, are zeroed by gdb_prepare and by the
 *   plan rebuild of a render call, and are left at zero by every completed render: one render at a time per workspace).
 *   (GDB_SCHED_AUTO takes DENSE for adaptive counts, FLAT where it measured faster: fp32, S_max <= 4, frames of few tiles per
 *   wave slot.  Both need the per-row plan + sample list in d_workspace: by default the render
 *   call builds them itself from frame->d_depth_range, a small launch of its own on the same stream — the one place a render
 *   call writes the workspace.  gdb_prepare builds the same plan inside its own launch when the frame it is given carries
 *   d_depth_range and the config is adaptive; a caller that has NOT changed the contents of d_depth_range since that
 *   gdb_prepare may OR GDB_SCHED_PLAN_READY into `schedule` to skip the rebuild.  With the flag set on a stale or missing plan
 *   the result is undefined but memory-safe: the kernel clamps everything it reads from the plan to the frame.)
 * Both are per-call arguments: the library keeps no process-global state (two engines with different settings may
 * interleave calls on different streams or threads).
 * Outputs d_bundle_feat (B*H*W, 3b²+C_f+3+C_v), d_depth, d_opacity (B*H*W).
 * bundle_size 1 and 4 (network.py:31-34; configs/dtu_pretrain.yaml:33 "4 for 4*4"; since round 6): TWO launches - the dense list kernel
 * on the bundles' CENTRE rays (everything of a sample but its 3b² sub-ray colours, which the MLP never sees: nerf.py:98), which also
 * leaves per (sample, view) the weight those colours get in the bundle's output (normalised composite weight x softmax blend weight,
 * utils.py:35-41, nerf.py:108-110), then k_bundle_colours: one thread per (bundle, sub-ray) gathers the colours with the reference's own
 * per-tap arithmetic (bundle_sampler.py:327-337) and assembles the rows.  `schedule` beyond its flags is ignored there (the one
 * schedule is DENSE), GDB_PREC_F32X runs the fp32 kernel; rows strips, batches and both output layouts as for bundle_size 2. */
#define GDB_PREC_F16 0
#define GDB_PREC_F32 1
#define GDB_PREC_F32X 2
#define GDB_SCHED_AUTO 0
#define GDB_SCHED_SLOT_WAVES 1
#define GDB_SCHED_SEGMENT_WAVE 2
#define GDB_SCHED_DENSE 3
#define GDB_SCHED_FLAT 4 /* (needs W x S_max < 65536, B x H < 65536, H x W < 2^24; GDB_E_SHAPE otherwise) */
#define GDB_SCHED_PLAN_READY 0x100 /* flag: the dense plan in d_workspace was built by gdb_prepare from the current d_depth_range */
#define GDB_SCHED_PYR16_READY 0x200 /* flag (GDB_PREC_F16): the half-precision pyramid in d_workspace was built by gdb_prepare_ex(GDB_PREP_PYR16)
                                     * for this frame; without it a GDB_PREC_F16 render first converts the fp32 pyramid (a launch of its own) */
int gdb_render_bundles_fused(const GdbConfig* cfg, const GdbFrame* frame, const void* d_workspace,
                             const float* d_packed_weights, int32_t row_begin, int32_t row_end,
                             int32_t precision, int32_t schedule, float* d_bundle_feat, float* d_depth,
                             float* d_opacity, void* stream);

/* What the two fused entries would do for this (config, frame shape, precision, row strip), without launching anything (ABI v6): the
 * library's own answer, so that no caller restates its rules.  shape needs B, V, Ho, Wo, H, W, D (no pointers).
 *   out[0]  1 when gdb_render_bundles_fused / _packed accept the config and frame (>= 2 source views; bundle_size 1, 2 or 4 since round
 *           6); 0: only the operator mirrors above run it (gdb_sample -> gdb_encode -> gdb_mlp -> gdb_composite).
 *   out[1]  the schedule GDB_SCHED_AUTO resolves to for this call (GDB_SCHED_SLOT_WAVES .. GDB_SCHED_FLAT; 0 when out[0] is 0).
 *   out[2]  1 when gdb_prepare builds the list schedules' plan for this config if the frame it is given carries d_depth_range - i.e. when a
 *           render of that frame may be passed GDB_SCHED_PLAN_READY (adaptive counts: while the contents of d_depth_range are unchanged).
 *   out[3]  kernel launches the render enqueues (1; one per batch item for the flat schedule and for a dense row strip of a batch; one
 *           more - k_bundle_colours - at bundle_size 1 / 4). */
int gdb_render_info(const GdbConfig* cfg, const GdbFrame* shape, int32_t precision, int32_t row_begin, int32_t row_end, int32_t out[4]);

/* The same with ONE output buffer d_out (B*H*W, Q+2), row = [bundle_feat (Q) | depth | opacity]: what
 * Network.render_bundles returns (network.py:54-91) as a single tensor, so that a row strip is one contiguous
 * block and the multi-GPU exchange is a single all-gather. */
int gdb_render_bundles_packed(const GdbConfig* cfg, const GdbFrame* frame, const void* d_workspace,
                              const float* d_packed_weights, int32_t row_begin, int32_t row_end,
                              int32_t precision, int32_t schedule, float* d_out, void* stream);

/* ---- "next" rows: the step just before the hot path ------------------------ */
/* build_feature_volume, networks/gdb_nerf/depth_net.py:424-476: plane-sweep warp of the source feature maps
 * d_src_feat (B,V,C,Hs,Ws) onto the target frustum planes d_depth_values (B,D,Ht,Wt) (depth or, with
 * inv_depth, disparity) + biased variance over views -> d_out (B,C,D,Ht,Wt).  Intrinsics are the
 * stage-scaled ones the reference passes.  d_proj_ws: B*V*12 floats of scratch. */
int gdb_build_feature_volume(const float* d_src_feat, const float* d_src_exts, const float* d_src_ints,
                             const float* d_tar_exts, const float* d_tar_ints, const float* d_depth_values,
                             int32_t B, int32_t V, int32_t C, int32_t Hs, int32_t Ws, int32_t D, int32_t Ht, int32_t Wt,
                             int32_t inv_depth, float* d_proj_ws, float* d_out, void* stream);

/* The same with scratch for a channel-pair re-layout of the source maps (ABI v5): d_pair_ws = B*V*C*Hs*Ws floats, or NULL (then
 * exactly gdb_build_feature_volume).  With it, an even C and V <= 4 the maps are first copied to [c/2][y][x][2] and the sweep takes
 * one 16-byte load per (channel PAIR, row, view) instead of two 8-byte ones: the kernel is bound by load instructions (texture
 * addresser), 48 -> 37 us at the DTU 256x320 stage including the copy.  Bit-identical results. */
int gdb_build_feature_volume_ws(const float* d_src_feat, const float* d_src_exts, const float* d_src_ints,
                                const float* d_tar_exts, const float* d_tar_ints, const float* d_depth_values,
                                int32_t B, int32_t V, int32_t C, int32_t Hs, int32_t Ws, int32_t D, int32_t Ht, int32_t Wt,
                                int32_t inv_depth, float* d_proj_ws, float* d_pair_ws, float* d_out, void* stream);

/* Backward of gdb_build_feature_volume (additions to ABI v7): from the forward's inputs and the upstream d_g_cost
 * (B,C,D,Ht,Wt) the gradients d_g_src_feat (B,V,C,Hs,Ws) and d_g_depth_values (B,D,Ht,Wt); either output may be NULL and is then
 * skipped (both NULL: GDB_E_BADARG).  The cameras get no gradient.  Coordinates, tap indices and weights are the forward's own bits.
 *   d_g_src_feat: d val_v = g (2/V)(val_v - mean), scattered through the forward's four tap weights (zeros padding), accumulated in
 *     64-bit fixed point - contributions scaled by 2^(F - e), e = ceil(log2 max|g_cost|) + ceil(log2 max|src_feat|) + 2,
 *     F = min(40, 62 - ceil(log2(4 D Ht Wt))), one integer atomic each, folded to float once: bit-identical from run to run.
 *   d_g_depth_values: one owner per element, fixed order; through the perspective divide with clamp_min(1e-6)'s derivative, times
 *     -1/h^2 under inv_depth; a view whose coordinate derivative is not finite adds nothing.
 *   max|g_cost| == 0 or max|src_feat| == 0: exact zeros.  Either not finite: both outputs are NaN.
 * Accepts every shape the forward accepts (V = 1 .. GDB_MAX_VIEWS, C >= 1, Ws >= 2, Hs >= 1); every refusal comes before the first
 * launch.  d_workspace: gdb_feature_volume_backward_workspace_bytes bytes (contents on entry do not matter; a call without
 * d_g_src_feat needs only 256 + 48 B V bytes rounded up to 256); a short one is GDB_E_WORKSPACE.  *out_frac_bits (may be NULL) = F.
 * No host synchronisation, no process-global state. */
int gdb_feature_volume_backward_workspace_bytes(int32_t B, int32_t V, int32_t C, int32_t Hs, int32_t Ws, int32_t D, int32_t Ht, int32_t Wt,
                                                size_t* out_bytes, int32_t* out_frac_bits);
int gdb_feature_volume_backward(const float* d_src_feat, const float* d_src_exts, const float* d_src_ints,
                                const float* d_tar_exts, const float* d_tar_ints, const float* d_depth_values, const float* d_g_cost,
                                int32_t B, int32_t V, int32_t C, int32_t Hs, int32_t Ws, int32_t D, int32_t Ht, int32_t Wt,
                                int32_t inv_depth, void* d_workspace, size_t ws_bytes, float* d_g_src_feat, float* d_g_depth_values,
                                void* stream);

/* depth_regression, depth_net.py:479-514: d_depth (B,1,H,W) soft-argmax of d_depth_values (B,D,H,W) under
 * d_depth_prob, d_ci (B,2,H,W) = mean -/+ ci_scale*std clipped to the hypothesis range (both returned as
 * depths when inv_depth). */
int gdb_depth_regression(const float* d_depth_values, const float* d_depth_prob, int32_t B, int32_t D, int32_t H, int32_t W,
                         float ci_scale, int32_t inv_depth, float* d_depth, float* d_ci, void* stream);

/* ---- merge around the decoder (next row N1) --------------------------------------------- */
/* network.py:170-182.  rgb_f = pixel_shuffle(bundle_feat[:, :3 b^2], b); img = rgb_c + rgb_f (rgb_c = the decoder's
 * (B,3,Ho,Wo) output, NULL = zeros); reweighting != 0: img = 0.5 (img + rgb_f).  d_out_depth / d_out_opacity
 * (B,Ho,Wo), either may be NULL: F.interpolate(scale_factor=b, mode='bilinear', align_corners=False) of the
 * (B,H,W) bundle maps.  shape needs B, H, W (Ho = H b, Wo = W b). */
int gdb_merge(const GdbConfig* cfg, const GdbFrame* shape, const float* d_bundle_feat, const float* d_rgb_c,
              const float* d_bundle_depth, const float* d_bundle_opacity, int32_t reweighting, float* d_img,
              float* d_out_depth, float* d_out_opacity, void* stream);
/* The same on the packed render of gdb_render_bundles_packed ((n_bundles, Q + 2) rows [bundle_feat | depth | opacity]), read in
 * place: the buffer a row-strip all-gather leaves on every rank (network.py:170-182 after the exchange of SURVEY.md 8(e)). */
int gdb_merge_packed(const GdbConfig* cfg, const GdbFrame* shape, const float* d_packed, const float* d_rgb_c, int32_t reweighting,
                     float* d_img, float* d_out_depth, float* d_out_opacity, void* stream);
/* (ABI v7, added) The image of gdb_merge_packed for the bundle rows [row_begin, row_end) only, written to d_tile (B,3,tile_rows*b,W*b)
 * from its row 0 (tile rows beyond the strip are left as they are): one rank's share of a frame decoded by row windows
 * (gdb_decode_rows; d_rgb_c is the frame-sized (B,3,H*b,W*b) buffer, only the strip's rows are read).  Bit-identical per pixel to
 * gdb_merge_packed.  gdb_upsample_maps: the depth / opacity upsampling of gdb_merge alone, on d_maps = B*H*W rows of map_stride
 * floats, depth in column 0 and opacity in column 1 (what a gather of the ranks' bundle-resolution maps leaves). */
int gdb_merge_packed_rows(const GdbConfig* cfg, const GdbFrame* shape, const float* d_packed, const float* d_rgb_c, int32_t reweighting,
                          int32_t row_begin, int32_t row_end, int32_t tile_rows, float* d_tile, void* stream);
int gdb_upsample_maps(const GdbConfig* cfg, const GdbFrame* shape, const float* d_maps, int32_t map_stride, float* d_out_depth,
                      float* d_out_opacity, void* stream);

/* ---- the decoder itself (next row N1) --------------------------------------------------- */
/* Decoder.forward, networks/gdb_nerf/decoder_rdn.py:44-81 (instantiated at network.py:51 as Decoder(C_f+3+C_v, 3, num_feats=64,
 * num_layers=nerf.dec_layers, upscale_factor=b); called at network.py:170-175): in_conv, num_layers ResidualDenseBlocks with
 * squeeze-excitation, up-conv + PixelShuffle, 1x1 out_conv — 3x3 convolutions as implicit GEMMs on fp32 MFMA, channel-last.
 * bundle_size 2 (upscale_factor 2: one up stage) and, since round 6, 4 (two up stages, decoder_rdn.py:59-62); bundle_size 1 (no up stage)
 * is refused; num_layers 1 .. 16 (two activation buffers alternate between the blocks).
 *
 * gdb_pack_decoder_weights: h_tensors in state-dict order — in_conv.weight (64,C_in,3,3), in_conv.bias, then per block
 * conv1.weight (32,64,3,3), conv2.weight (32,96,3,3), conv3.weight (64,128,3,3), se.fc.0.weight (4,64), se.fc.2.weight (64,4),
 * then up.0.weight (256,64,3,3), up.0.bias, [bundle_size 4: up.2.weight (256,64,3,3), up.2.bias,] out_conv.weight (3,64,1,1),
 * out_conv.bias: 2 + 5 num_layers + 4 (+ 2) host pointers.
 * The LAST up stage is folded with out_conv into one 64 -> 12 convolution on the host (no non-linearity sits between up-conv,
 * PixelShuffle and out_conv); at bundle_size 4 the first up stage runs as four 64 -> 64 convolutions, one per sub-pixel of its
 * PixelShuffle, into a (2H, 2W, 64) map in the workspace, on which the folded stage then runs: d_rgb_c is (B, 3, 4H, 4W). */
int gdb_decoder_packed_floats(const GdbConfig* cfg, int32_t num_layers, size_t* out_floats);
int gdb_pack_decoder_weights(const GdbConfig* cfg, int32_t num_layers, const float* const* h_tensors, float* h_out);
/* shape needs B, H, W (the bundle map). */
int gdb_decoder_workspace_bytes(const GdbConfig* cfg, const GdbFrame* shape, size_t* out_bytes);
/* d_bundle_feat: the hot path's output rows (B*H*W, ld_bundle_feat >= Q), read in place: the decoder's input is channels
 * 3b² .. Q-1 of every row (network.py:170-174: nerf_feat[:, 3b²:]).  d_rgb_c (B,3,H*b,W*b) = the reference's `rgb_c`; feed it
 * to gdb_merge.  d_workspace: gdb_decoder_workspace_bytes, caller-owned scratch.
 * precision: GDB_PREC_F32 (fp32 MFMA, the reference's arithmetic) or GDB_PREC_F32X (split-f16 operand pairs, fp32 accumulate:
 * fp32-grade, the convolutions' matrix time 5.3x shorter); the packed weights hold both forms.  The decoder's pairs - stored
 * activations and weights alike - are hi = f16(v), lo = f16(v - hi), both to nearest even (activations clamped to +-65504 first), a
 * product hi*hi + hi*lo + lo*hi with fp32 accumulate: the operand range of gdb_render_bundles_fused's GDB_PREC_F32X text applies, an
 * operand below 2^-3 keeps an absolute 2^-25 (DESIGN.md section 4.11 has the contract and its float64 referee). */
int gdb_decode(const GdbConfig* cfg, const GdbFrame* shape, const float* d_bundle_feat, int32_t ld_bundle_feat,
               const float* d_packed_decoder_weights, int32_t num_layers, int32_t precision, void* d_workspace,
               size_t workspace_bytes, float* d_rgb_c, void* stream);

/* ---- the decoder by row windows (ABI v7, added) -------------------------------------------- */
/* The decode of the bundle-map rows [row_begin, row_end) alone, for a frame whose rows are split over ranks.  The library holds no
 * communicator, so the decode returns to the caller at every squeeze-excitation (its mean runs over the whole image): phase p of
 * 0 .. num_layers first runs the gate of block p-1 (p > 0) on the workspace's frame-sized channel-sum buffer `part`, then block p's
 * three convolutions (in_conv first when p = 0; their sums are written to `part` for the owned rows only, at their frame row), and
 * phase num_layers the up stage(s), writing rows [row_begin*b, row_end*b) of the frame-sized d_rgb_c (B,3,H*b,W*b) only (d_rgb_c may
 * be NULL before that phase).  Between phases the caller fills the other rows of `part` (an all-gather of every rank's owned rows).
 * The convolutions run on a window [row_begin - h, row_end + h) ∩ [0, H), start rounded down to a multiple of 4, with
 * h = 1 + 3 num_layers + log2(b) rows: d_bundle_feat (frame-sized, as for gdb_decode) must hold the window's rows.  The rows
 * written are bit-identical to gdb_decode's on the whole frame, at both precisions.
 * gdb_decoder_rows_layout: the byte offset of `part` in the workspace and its row pitch (part is (B, H, pitch) floats: item b, row y
 * at offset + (b H + y) pitch_bytes), and the window [*window_begin, *window_end); any out pointer may be NULL. */
int gdb_decoder_rows_workspace_bytes(const GdbConfig* cfg, const GdbFrame* shape, int32_t row_begin, int32_t row_end,
                                     int32_t num_layers, size_t* out_bytes);
int gdb_decoder_rows_layout(const GdbConfig* cfg, const GdbFrame* shape, int32_t row_begin, int32_t row_end, int32_t num_layers,
                            size_t* part_offset, size_t* part_row_bytes, int32_t* window_begin, int32_t* window_end);
int gdb_decode_rows(const GdbConfig* cfg, const GdbFrame* shape, const float* d_bundle_feat, int32_t ld_bundle_feat,
                    const float* d_packed_decoder_weights, int32_t num_layers, int32_t precision, int32_t row_begin, int32_t row_end,
                    int32_t phase, void* d_workspace, size_t workspace_bytes, float* d_rgb_c, void* stream);
/* gdb_decoder_rows_regions (ABI v7, added; host only, launches nothing): the fp32 regions of that workspace, GDB_DEC_REGIONS of them in
 * this order - "P0", "P1", "P2" (block inputs x_b, (B, Hw, W, 64) over the window's Hw rows; block_input[b], b = 0 .. num_layers-1, is
 * the index of the P that holds x_b: P0 = in_conv's output and the global residual), "Y" ([x1 | x2] of the block in flight), "T" (its
 * conv3), "part" ((B, H, ceil(W/32), 64): channel sums of T per frame row and 32-pixel segment), "part2" ((B, groups, 64)), "gate"
 * ((B, 64)), and at bundle_size 4 "X" ((B, Hw, W, 64): the blocks' output with the last gate and the global residual applied) and "U"
 * ((B, 2Hw, 2W, 64): the first up stage) - both of zero bytes at bundle_size 2.  shape: unused trailing dimensions are 0.  out may be
 * NULL to query *out_count; block_input may be NULL.  After phase p of a window equal to the frame the regions hold x_p, Y, T and part
 * of block p and the gate of block p-1 (after phase num_layers: the last gate, and X / U). */
#define GDB_DEC_REGIONS 10
typedef struct GdbDecRegion {
    char name[16];
    uint64_t offset;    /* bytes from the start of the workspace */
    uint64_t bytes;
    int32_t shape[4];
} GdbDecRegion;
int gdb_decoder_rows_regions(const GdbConfig* cfg, const GdbFrame* shape, int32_t row_begin, int32_t row_end, int32_t num_layers,
                             GdbDecRegion* out, int32_t capacity, int32_t* out_count, int32_t* block_input);

/* ---- the decoder in training mode: device-side pack, saved-activation forward, backward (ABI v7, added) ---------- */
/* fp32 only (precision must be GDB_PREC_F32), bundle_size 2, num_layers 1 .. 16, B <= 256, whole frames: every entry refuses anything
 * else.
 *
 * gdb_decoder_train_pack: d_tensors = DEVICE pointers to the parameters in the state-dict order of gdb_pack_decoder_weights
 * (2 + 5 num_layers + 4).  Two launches on `stream` write d_packed (gdb_decoder_train_packed_floats floats): the fp32 operand forms at
 * the offsets of the eval-mode packed buffer's fp32 sections, byte for byte what gdb_pack_decoder_weights writes from the same values
 * (the last up stage folded with out_conv in double, in the host's order, rounded once), then a zeroed tap block, then the
 * data-gradient forms the backward's convolutions read (channel roles swapped, taps flipped).  No parameter is copied
 * to the host and nothing synchronises.  gdb_decode(GDB_PREC_F32) accepts the buffer too; the split-f16 forms are not in it.
 *
 * gdb_decoder_train_forward: gdb_decode's fp32 launch sequence with every block's activations kept in d_saved
 * (gdb_decoder_train_saved_bytes): d_rgb_c (B,3,2H,2W) is bit-identical to gdb_decode(..., GDB_PREC_F32, ...) on the same inputs.
 * gdb_decoder_train_layout (host only) names the regions, 4 num_layers + 3 of them: per block b "x.<b>" (its input, (B, H, W, 64);
 * x.0 = shallow = in_conv's output), "ab.<b>" ([a | b] = conv1 | conv2 after ReLU, 32 + 32 channels), "T.<b>" (conv3's output),
 * "gate.<b>" ((B, 64)); then "xu" (the up stage's input x_L + shallow, x_L = x_{L-1} + T gate), "part" ((B, H, ceil(W/32), 64): the last
 * block's channel sums of T per row and 32-pixel segment) and "part2" ((B, groups, 64)).  out may be NULL to query *out_count. */
int gdb_decoder_train_packed_floats(const GdbConfig* cfg, int32_t num_layers, size_t* out_floats);
int gdb_decoder_train_pack(const GdbConfig* cfg, int32_t num_layers, int32_t precision, const float* const* d_tensors, float* d_packed,
                           size_t packed_floats, void* stream);
int gdb_decoder_train_saved_bytes(const GdbConfig* cfg, const GdbFrame* shape, int32_t num_layers, size_t* out_bytes);
int gdb_decoder_train_layout(const GdbConfig* cfg, const GdbFrame* shape, int32_t num_layers, GdbDecRegion* out, int32_t capacity,
                             int32_t* out_count);
int gdb_decoder_train_forward(const GdbConfig* cfg, const GdbFrame* shape, const float* d_bundle_feat, int32_t ld_bundle_feat,
                              const float* d_packed, int32_t num_layers, int32_t precision, void* d_saved, size_t saved_bytes,
                              float* d_rgb_c, void* stream);
/* gdb_decoder_train_backward: from d_g_rgb_c (B,3,2H,2W), the saved buffer of the forward on the same rows and packed weights, and
 * the parameters themselves (d_tensors, as for the pack: the fold's backward reads up.0 and out_conv), the gradient of every parameter
 * in that parameter's own layout - d_grads: 2 + 5 num_layers + 4 device pointers in state-dict order, any of them NULL (or d_grads
 * NULL) - and of the bundle rows: d_g_rows (B H W, ld_g_rows >= Q), columns 12 .. 38 the gradient, 0 .. 11 written as zero, columns
 * from 39 on left alone; may be NULL.  Everything is overwritten, not accumulated.  d_workspace: gdb_decoder_train_backward_bytes,
 * caller-owned scratch.  No atomics on data: two runs are bit-identical. */
int gdb_decoder_train_backward_bytes(const GdbConfig* cfg, const GdbFrame* shape, int32_t num_layers, size_t* out_bytes);
int gdb_decoder_train_backward(const GdbConfig* cfg, const GdbFrame* shape, const float* d_bundle_feat, int32_t ld_bundle_feat,
                               const float* d_packed, int32_t num_layers, int32_t precision, const float* const* d_tensors,
                               const void* d_saved, size_t saved_bytes, const float* d_g_rgb_c, void* d_workspace, size_t workspace_bytes,
                               float* const* d_grads, float* d_g_rows, int32_t ld_g_rows, void* stream);

/* ---- the decoder on plain f16 MFMA with half-precision activations (ABI v7, added) ---------- */
/* The same network (bundle_size 2, feat_dim 16, voxel_dim 8, num_layers 1 .. 16) under a narrower, explicit contract: weights f16(w)
 * (the up stage folded with out_conv in fp64, then rounded once), biases fp32; the 27 input channels read in place from the fp32 rows
 * and rounded to f16; every convolution f16 x f16 with fp32 accumulate, bias and ReLU in fp32, ONE rounding to f16, stored
 * channel-last in the workspace; squeeze-excitation sums from conv3's unrounded accumulators, gate in fp32; trunk update
 * x <- f16(fma(c, gate, x)) and global residual f16(shallow + trunk) materialised; the folded 64 -> 12 convolution writes fp32 d_rgb_c
 * (B,3,2H,2W).  Deterministic, no atomics on data, workspace contents never matter.  gdb_decode / gdb_decode_rows keep refusing
 * GDB_PREC_F16: this form has its own packed buffer and entries.
 *
 * Packed buffer (gdb_decoder_f16_packed_bytes; h_tensors as for gdb_pack_decoder_weights): a convolution of nct 16-channel output
 * tiles and nks 32-channel K-steps is nct*nks*9*64*16 bytes, [tile][K-step][tap 9][lane 64][8 halves], element j of lane l =
 * f16(W[16 tile + (l & 15)][32 kstep + 8 (l >> 4) + j][tap]), zero beyond the layer's channels.  Sections in order: in_conv (nct 4,
 * nks 1), in_conv.bias (64 floats); per block conv1 (2, 2), conv2 (2, 3), conv3 (4, 4), se.fc.0 (4 x 64 floats), se.fc.2 (64 x 4
 * floats); the folded up stage (1, 2), channel 3 s + o of sub-pixel s = dy*2 + dx, and its bias (64 floats, 12 used).
 *
 * flags: GDB_DECF16_KEEP_LAYERS gives every layer's output, every gate and every trunk a workspace region of its own (without it
 * two trunk buffers alternate between the blocks and conv1 / conv2 / conv3 / gate regions are shared); d_rgb_c is bit-identical
 * either way.  gdb_decoder_f16_layout lists the regions (out may be NULL to query *out_count = 5 num_layers + 2): "trunk.<b>"
 * (b = 0 .. num_layers: the input of block b; trunk.0 = in_conv's output, trunk.<num_layers> = the blocks' output),
 * "blocks.<b>.conv1" / ".conv2" (32 channels) / ".conv3" (64), "blocks.<b>.gate" (64 floats per batch item: per_pixel 0),
 * "residual" (= f16(trunk.0 + trunk.<num_layers>), the up stage's input).  Per-pixel regions are (B*H*W, channels) rows.
 * Refused before the first launch: bundle_size != 2, num_layers outside 1 .. 16, feat_dim / voxel_dim other than 16 / 8, unknown
 * flags (GDB_E_BADARG); a short row stride or non-positive map (GDB_E_SHAPE); a short workspace (GDB_E_WORKSPACE); NULL pointers. */
#define GDB_DECF16_KEEP_LAYERS 1
#define GDB_DECF16_T_F16 0
#define GDB_DECF16_T_F32 1
typedef struct GdbDecF16Region {
    char name[32];
    uint64_t offset;    /* bytes from the start of the workspace */
    int32_t channels;
    int32_t dtype;      /* GDB_DECF16_T_* */
    int32_t per_pixel;  /* 1: (B*H*W, channels); 0: (B, channels) */
    int32_t reserved;
} GdbDecF16Region;
int gdb_decoder_f16_packed_bytes(const GdbConfig* cfg, int32_t num_layers, size_t* out_bytes);
int gdb_pack_decoder_weights_f16(const GdbConfig* cfg, int32_t num_layers, const float* const* h_tensors, void* h_out);
int gdb_decoder_f16_workspace_bytes(const GdbConfig* cfg, const GdbFrame* shape, int32_t num_layers, int32_t flags, size_t* out_bytes);
int gdb_decoder_f16_layout(const GdbConfig* cfg, const GdbFrame* shape, int32_t num_layers, int32_t flags, GdbDecF16Region* out,
                           int32_t capacity, int32_t* out_count);
int gdb_decode_f16(const GdbConfig* cfg, const GdbFrame* shape, const float* d_bundle_feat, int32_t ld_bundle_feat,
                   const void* d_packed_f16, int32_t num_layers, int32_t flags, void* d_workspace, size_t workspace_bytes,
                   float* d_rgb_c, void* stream);

/* ---- the cascade's cost-regularisation 3-D U-Nets (ABI v7, added) ---------------------------- */
/* _UNet3d.forward, networks/gdb_nerf/cost_reg_net.py:24-54, eval mode: depth 2 (CostRegNet_small) or 3 (CostRegNet), in_channels cin
 * (a multiple of 8, <= 256), base_channels (a multiple of 8, base << depth <= 128), out_channels cout = voxel_dim (1 .. 15).  Every
 * 3x3x3 (transposed) convolution on fp32 MFMA with eval BatchNorm + ReLU (+ the skip add) fused; activations channel-last in the
 * caller's workspace.
 *
 * gdb_pack_cost_reg_weights: h_tensors in this order - for i = 0 .. 3 depth: conv{i}.0.weight, conv{i}.1.weight, conv{i}.1.bias,
 * conv{i}.1.running_mean, conv{i}.1.running_var; then feat_head.weight, prob_head.weight, and a pointer to the BatchNorm eps (one
 * float): 5 (3 depth + 1) + 3 host pointers.  Packed layer L (conv0 .. conv{3 depth}, then the heads) holds its weights at
 * w_off(L) + (((mt T + tap) K + cc) 64 + lane) E + e = weight of GEMM row 16 mt + (lane & 15), input channel ci, tap; T = 27
 * (tap = (kz 3 + ky) 3 + kx) or 36 for the 8-channel stride-1 layers (rows 8 .. 15 = the same channels one plane further),
 * ci = 16 cc + 4 e + (lane >> 4) with E = 4 for conv0, else ci = 4 E cc + E (lane >> 4) + e with E = 4 (cin % 16 == 0) or 2; the
 * heads' rows are feat_head 0 .. cout - 1 and prob_head cout.  A BN layer's weights are followed by [1 / sqrt(var + eps) | mean |
 * weight | bias] x its cout; each block starts at a multiple of 64 floats.
 * gdb_cost_reg_workspace_bytes / gdb_cost_reg: d_cost (B, cin, D, H, W) as gdb_build_feature_volume writes it, read in place; D, H
 * and W divisible by 2^depth (GDB_E_SHAPE otherwise), ws_bytes >= the workspace size (GDB_E_WORKSPACE otherwise; its contents do
 * not matter).  Out: d_volume (B, cout, D, H, W), d_prob (B, D, H, W) = softmax over D of prob_head.  Every refusal comes before
 * the first launch.  Deterministic (no atomics).
 * The workspace is the caller's, and after the call it still holds every intermediate, channel-last, in this order:
 *   S_0 | S_1 T_1 | ... | S_depth T_depth,   S_l and T_l: (B, D >> l, H >> l, W >> l, base << l) floats, each rounded up to a
 *   multiple of 64 floats (the padding is never written); the byte count is 4 x the sum (no T_0).
 * T_l (l >= 1) is the output of the stride-2 conv(2l - 1).  S_depth is the output of the deepest stride-1 layer, conv(2 depth).
 * S_l for l < depth was the skip (conv0, or conv(2l)) and is left in its final state, skip + the transposed convolution that
 * writes level l (conv(3 depth - l)): the value the next layer up, or for l = 0 the two heads, read.  The skips themselves are
 * overwritten by that add. */
int gdb_cost_reg_packed_floats(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, size_t* out_floats);
int gdb_pack_cost_reg_weights(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* const* h_tensors, float* h_out);
int gdb_cost_reg_workspace_bytes(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, int32_t B, int32_t D, int32_t H,
                                 int32_t W, size_t* out_bytes);
int gdb_cost_reg(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* d_cost, int32_t B, int32_t D, int32_t H,
                 int32_t W, const float* d_packed, void* d_workspace, size_t ws_bytes, float* d_volume, float* d_prob, void* stream);

/* ---- the feature pyramid network (ABI v7, added) --------------------------------------------------------------------------- */
/* FeatureNet.forward, networks/gdb_nerf/feature_net.py, eval mode: base_channels c (a multiple of 8, <= 32), out_channels out0, out1,
 * out2 (multiples of 8, <= 64).  Every convolution on fp32 MFMA with eval BatchNorm + ReLU, or the bias and the upsampled add of the
 * top-down path, fused; intermediates channel-last in the caller's workspace.
 *
 * gdb_pack_fpn_weights: h_tensors in this order - for conv0.0, conv0.1, conv1.0, conv1.1, conv2.0, conv2.1: X.0.weight, X.1.weight,
 * X.1.bias, X.1.running_mean, X.1.running_var; then out0.weight, out0.bias, inner1.weight, inner1.bias, inner2.weight, inner2.bias,
 * out1.weight, out2.weight, and a pointer to the BatchNorm eps (one float): 39 host pointers.  Packed layers, in the order conv0.0,
 * conv0.1, conv1.0, conv1.1, conv2.0, conv2.1, out0, inner1, inner2, out1, out2, hold their weights at
 * w_off(L) + (((mt T + tap) K + cc) 64 + lane) E + e = weight of GEMM row 16 mt + (lane & 15), with
 *  - conv0.0 (3 input channels): E = 1, K = 1, T = 7 (9 when c == 8) k-steps; k = 4 tap + (lane >> 4) = (ci R + r) 3 + kx over
 *    R = 3 (4) input rows r, ky = r - (row >> 3) when c == 8, else ky = r; zeros for k >= 9 R or ky outside 0 .. 2;
 *  - every other layer: ci = 4 E cc + E (lane >> 4) + e with E = 4 (cin % 16 == 0) or 2, K = cin / (4 E); tap = ky ks + kx (ks = 5
 *    for conv1.0 / conv2.0, 1 for out0 / inner*, else 3), except for 3x3 layers with 8 output channels: T = 12, tap = r 3 + kx
 *    over 4 input rows r, ky = r - (row >> 3);
 *  - GEMM row = output channel, or for the 8-output-channel 3x3 layers row = 8 s + channel with s = the output row y + s; zeros for
 *    rows >= that count.
 * Each layer's weights are followed by [1 / sqrt(var + eps) | mean | weight | bias] x its cout (conv blocks) or its bias x cout
 * (out0, inner1, inner2); out1 and out2 have none; each block starts at a multiple of 64 floats.
 * gdb_fpn_workspace_bytes / gdb_fpn: d_images (N, 3, H, W), read in place; N, H, W >= 1 (GDB_E_SHAPE otherwise); level_mask: bit l
 * asks for level l (a non-empty subset of 0 .. 2, GDB_E_BADARG otherwise); ws_bytes >= the workspace size for that mask
 * (GDB_E_WORKSPACE otherwise; its contents do not matter).  With h = ceil(H / 2), q = ceil(h / 2) (and so for W), out: d_level0
 * (N, out0, q, wq), d_level1 (N, out1, h, w), d_level2 (N, out2, H, W); a level's pointer may be NULL exactly when the mask leaves
 * it out.  Only what the mask needs runs: the encoder always, inner1 for levels 1 or 2, inner2 and out2 for level 2.  Every refusal
 * comes before the first launch.  Deterministic (no atomics).
 * The workspace is the caller's, and after the call it still holds the intermediates, channel-last (N, rows, columns, channels),
 * in this order, each region rounded up to a multiple of 64 floats (the padding is never written); the byte count is 4 x the sum:
 *   A  (N, H, W, c)    conv0.0's output      - only when the mask leaves level 2 out; with level 2 it is written into I2's space
 *                                              and overwritten there by inner2 (I2 is first written after A is last read)
 *   F0 (N, H, W, c)    conv0 = conv0.1's output          T1, H1 (N, h, w, 2c)   conv1.0's and conv1.1's outputs
 *   T2, Q (N, q, wq, 4c)  conv2.0's and conv2.1's outputs
 *   I1 (N, h, w, 4c)   interpolate(Q) + inner1(H1)       - only with level 1 or 2 in the mask
 *   I2 (N, H, W, 4c)   interpolate(I1) + inner2(F0)      - only with level 2 in the mask
 * out0 reads Q, out1 reads I1, out2 reads I2.  A run with mask 3 and one with mask 7 on the same images between them leave every
 * layer's input and output; the regions they share are bit-identical (tests/test_fpn_referee.py reads them back this way). */
int gdb_fpn_packed_floats(int32_t base_channels, int32_t out0, int32_t out1, int32_t out2, size_t* out_floats);
int gdb_pack_fpn_weights(int32_t base_channels, int32_t out0, int32_t out1, int32_t out2, const float* const* h_tensors, float* h_out);
int gdb_fpn_workspace_bytes(int32_t base_channels, int32_t out0, int32_t out1, int32_t out2, int32_t N, int32_t H, int32_t W,
                            int32_t level_mask, size_t* out_bytes);
int gdb_fpn(int32_t base_channels, int32_t out0, int32_t out1, int32_t out2, const float* d_images, int32_t N, int32_t H, int32_t W,
            const float* d_packed, int32_t level_mask, void* d_workspace, size_t ws_bytes, float* d_level0, float* d_level1,
            float* d_level2, void* stream);

/* ---- the evaluator's metrics (ABI v7, added) -------------------------------------------------------------------------------- */
/* What evaluators/gdb_nerf.py computes per frame, on the device: every call enqueues its launches on `stream` and leaves one record
 * of doubles per batch item; nothing is copied to the host and nothing waits.  All arithmetic in fp64 from the fp32 inputs.  Record b
 * is written at d_records + b * record_stride (record_stride in doubles, at least the record's length), so records can go straight
 * into the rows of a larger table.  Deterministic: per-workgroup partial sums in d_workspace, added in a fixed order by a second
 * launch, no atomics; the workspace's and the records' previous contents do not matter.
 * gdb_eval_workspace_bytes: enough for either call on B images or ground-truth depth maps of H x W.
 * gdb_eval_image: d_pred (B, 3, H, W) as Network.forward returns it (clamped to [0, 1] here), d_gt (B, H, W, 3), d_mask (B, H, W) with
 * the rule mask >= 1, all read in place; the crop is rows [crop_y0, crop_y0 + crop_h), columns [crop_x0, crop_x0 + crop_w) of the
 * image (0, 0, H, W for all of it).  Record (GDB_EVAL_IMAGE_REC doubles): [sum of (gt - pred)^2 over the masked pixels' three
 * channels, masked pixels, then per channel the sum of the SSIM map over the (crop_h - 6) x (crop_w - 6) windows that lie inside the
 * crop, of the images zeroed outside the mask]; SSIM per window: 7 x 7 means, sample covariance (x 49 / 48), K1 0.01, K2 0.03, data
 * range 2.  GDB_E_SHAPE for B, H or W < 1, a crop outside the image or one with fewer than 7 rows or columns.
 * gdb_eval_depth: d_depth (B, Hd, Wd) against d_gt (B, H, W) over the pixels with gt != 0; resize != 0 resamples d_depth to H x W
 * (bilinear, half-pixel centres, edge clamp, i.e. cv2.INTER_LINEAR), resize == 0 needs Hd == H and Wd == W (GDB_E_SHAPE otherwise).
 * Record (GDB_EVAL_DEPTH_REC doubles): [sum of |err|, count(|err| < 2), count(|err| < 10), count(gt != 0)].
 * GDB_E_BADARG for a NULL pointer or a short record_stride, GDB_E_WORKSPACE for a short workspace; every refusal comes before the
 * first launch. */
#define GDB_EVAL_IMAGE_REC 5
#define GDB_EVAL_DEPTH_REC 4
int gdb_eval_workspace_bytes(int32_t B, int32_t H, int32_t W, size_t* out_bytes);
int gdb_eval_image(const float* d_pred, const float* d_gt, const float* d_mask, int32_t B, int32_t H, int32_t W, int32_t crop_y0,
                   int32_t crop_x0, int32_t crop_h, int32_t crop_w, void* d_workspace, size_t ws_bytes, double* d_records,
                   int64_t record_stride, void* stream);
int gdb_eval_depth(const float* d_depth, int32_t Hd, int32_t Wd, const float* d_gt, int32_t B, int32_t H, int32_t W, int32_t resize,
                   void* d_workspace, size_t ws_bytes, double* d_records, int64_t record_stride, void* stream);

/* ---- LPIPS with the VGG-16 backbone, from caller-supplied weights (ABI v7, added) --------------------------------------------
 * lpips.LPIPS(net='vgg') in eval mode, spatial=False, as of release 0.1.4, restated (the package is not available to this project: the
 * definition here is the contract, and agreement with the package's published weights and values is unverified).  For two images a, b
 * with values in [0, 1], shape (3, h, w):
 *   1. scaling layer: x = ((2 img - 1) - shift_c) / scale_c per channel (the package's shift [-.030, -.088, -.188], scale [.458, .448, .450]);
 *   2. thirteen 3 x 3 convolutions, stride 1, with bias and ReLU, zero padding 1 applied to the SCALED input; channels 3->64, 64->64 |
 *      64->128, 128->128 | 128->256, 256->256 x 2 | 256->512, 512->512 x 2 | 512->512 x 3; a 2 x 2 stride-2 max-pool between the groups,
 *      floor (an odd last row or column is dropped);
 *   3. taps: the five group outputs after ReLU and before the pool (relu1_2, 2_2, 3_3, 4_3, 5_3);
 *   4. per tap l and pixel: n = sqrt(sum_c f_c^2) + 1e-10 (the eps outside the root), d = sum_c w_lc (fa_c / na - fb_c / nb)^2 with the
 *      tap's 1 x 1 weights w_l (C_l values, no bias); t_l = the mean of d over the tap's pixels;
 *   5. LPIPS = sum_l t_l.
 * Per-pixel terms in fp32 (convolutions on fp32 MFMA: exact products, fp32 accumulate), sums over pixels and taps in fp64 in a fixed
 * order: deterministic, no atomics, the workspace's previous contents do not matter, and an image's value does not depend on its
 * batch position.  Nothing syncs with the host; the library allocates nothing.
 *
 * gdb_pack_lpips_weights (host side): h_tensors = 13 convolution weights (cout, cin, 3, 3), their 13 biases, the 5 tap weights (C_l
 * floats), shift (3), scale (3): GDB_LPIPS_TENSORS host pointers, none NULL (GDB_E_BADARG).  Packed buffer (gdb_lpips_packed_floats),
 * every block at a multiple of 64 floats: [shift 3 | scale 3]; conv.0 weights [mt 4][step 7][lane 64] = W[16 mt + (lane & 15)][k = 4 step
 * + (lane >> 4)], k = (ci 3 + ky) 3 + kx, zero at k = 27, and its bias; conv.i weights [mp cout / 32][tap 9][cc cin / 16][m 2][lane 64][e 4]
 * = W[32 mp + 16 m + (lane & 15)][16 cc + 4 (lane >> 4) + e][tap = ky 3 + kx], and its bias; then the five tap weights.
 *
 * gdb_eval_lpips: d_pred (B, 3, H, W), d_gt (B, H, W, 3), d_mask (B, H, W), read in place as gdb_eval_image reads them: the crop, the
 * clamp of d_pred to [0, 1], both images zeroed except where mask >= 1 (the evaluator's rule: a NaN mask value counts as masked; image value 0, i.e. -1 before the scaling layer) and the scaling
 * layer are applied by the first convolution on load.  Writes ONE double per batch item at d_records + b * record_stride.
 * Activations are channel-last fp32 (2 B, rows, columns, channels): image n < B is d_pred of item n, image B + n is d_gt of item n.
 * flags 0: two activation buffers alternate.  GDB_LPIPS_KEEP: the scaled input, every convolution's output and the four pooled maps
 * each keep a region of their own; the record is bit-identical either way.  gdb_lpips_layout lists the regions of a workspace (h, w:
 * the cropped extent; out may be NULL to query *out_count): with GDB_LPIPS_KEEP "scaled", then "conv.0", "conv.1", "pool.0", "conv.2",
 * ... "conv.12" in the order they are written, else "ping", "pong"; then "taps" ((B, 5) doubles: the t_l) and "partials" (doubles).
 * Refused before any launch: a NULL pointer, unknown flags or a record_stride < 1 (GDB_E_BADARG); B, H or W < 1, a crop outside the
 * image, a cropped extent below 16 rows or columns - the fifth tap would be empty (GDB_E_SHAPE); a short workspace (GDB_E_WORKSPACE). */
#define GDB_LPIPS_KEEP 1
#define GDB_LPIPS_TENSORS 33
#define GDB_LPIPS_REGIONS 20
int gdb_lpips_packed_floats(size_t* out_floats);
int gdb_pack_lpips_weights(const float* const* h_tensors, float* h_out);
int gdb_lpips_workspace_bytes(int32_t B, int32_t h, int32_t w, int32_t flags, size_t* out_bytes);
int gdb_lpips_layout(int32_t B, int32_t h, int32_t w, int32_t flags, GdbDecRegion* out, int32_t capacity, int32_t* out_count);
int gdb_eval_lpips(const float* d_pred, const float* d_gt, const float* d_mask, int32_t B, int32_t H, int32_t W, int32_t crop_y0,
                   int32_t crop_x0, int32_t crop_h, int32_t crop_w, const float* d_packed, int32_t flags, void* d_workspace,
                   size_t workspace_bytes, double* d_records, int64_t record_stride, void* stream);

/* ---- one cascade MVS stage as one call (ABI v7, added) ------------------------------------------------------------------------
 * One stage of DepthNet.forward (networks/gdb_nerf/depth_net.py:133-156): camera set-up, plane sweep, the stage's U-Net, softmax
 * over D and depth regression.  Nothing syncs with the host; deterministic (no atomics); the caller owns all memory.
 *
 * Search range d_range (B, 2, hr, wr), channel 0 = lo, 1 = hi (depths).  hr = wr = 1: broadcast over the target (stage 0's
 * near / far; `ratio` is ignored).  Otherwise the previous stage's interval: pixel (y, x) of the (Ht, Wt) target takes the bilinear
 * sample F.interpolate(scale_factor = ratio, mode = "bilinear", align_corners = False) takes, src = max((dst + 0.5) / ratio - 0.5, 0),
 * neighbours clamped to the last row / column (a target larger than ratio x (hr, wr) repeats the last sample).  The hypothesis of
 * plane d is lo' + (hi' - lo') * step_d, lo' / hi' the sampled ends or, with inv_depth, their reciprocals, step_d =
 * torch.linspace(0, 1, D)[d] in fp32; every multiply-add rounds twice, as the separate torch ops do.
 *
 * gdb_mvs_hypotheses writes these (B, D, Ht, Wt) hypotheses to d_out: a test and diagnosis entry, the stage never materialises them.
 *
 * gdb_mvs_stage: d_src_feat (B, V, C, Hs, Ws); d_src_exts (B, V, 4, 4), d_src_ints (B, V, 3, 3), d_tar_exts (B, 4, 4), d_tar_ints
 * (B, 3, 3) with the UNSCALED intrinsics: rows 0-1 are multiplied by feat_scale (source) / vol_scale (target) in fp32 before the
 * projection products, as `K[..., :2, :] *= s` does.  The U-Net is (depth, cin = C, base_channels, cout) with d_packed in
 * gdb_pack_cost_reg_weights' format; D, Ht and Wt divisible by 2^depth, D <= 512.  Out: d_volume (B, cout, D, Ht, Wt) the feat
 * head's output, d_depth (B, Ht, Wt), d_ci (B, 2, Ht, Wt) = mean -/+ ci_scale * std clipped to the hypothesis range (depths), and
 * d_vol_range (B, 2, Ht, Wt) = the first and last hypothesis (disparities under inv_depth, as depth_net.py:153 returns them).  The
 * softmax probabilities are never written.  ws_bytes >= gdb_mvs_stage_workspace_bytes (GDB_E_WORKSPACE otherwise); the workspace's
 * contents do not matter.  Every refusal comes before the first launch. */
int gdb_mvs_stage_workspace_bytes(int32_t B, int32_t V, int32_t C, int32_t Hs, int32_t Ws, int32_t D, int32_t Ht, int32_t Wt,
                                  int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, size_t* out_bytes);
int gdb_mvs_stage(const float* d_src_feat, const float* d_src_exts, const float* d_src_ints, const float* d_tar_exts,
                  const float* d_tar_ints, float feat_scale, float vol_scale, const float* d_range, int32_t hr, int32_t wr, double ratio,
                  int32_t B, int32_t V, int32_t C, int32_t Hs, int32_t Ws, int32_t D, int32_t Ht, int32_t Wt, int32_t inv_depth,
                  float ci_scale, int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* d_packed,
                  void* d_workspace, size_t ws_bytes, float* d_volume, float* d_depth, float* d_ci, float* d_vol_range, void* stream);
int gdb_mvs_hypotheses(const float* d_range, int32_t hr, int32_t wr, double ratio, int32_t B, int32_t D, int32_t Ht, int32_t Wt,
                       int32_t inv_depth, float* d_out, void* stream);

/* ---- the training loss: MSE + SSIM value and gradient, and the depth monitor (ABI v7, added) ---------------------------------
 * The photometric loss of train/losses/gdb_nerf.py without its perceptual term, as one call that leaves the value and the gradient
 * with respect to the estimate on the device.  Nothing is copied to the host, nothing waits, the library allocates nothing.
 *
 * Definition, all per-pixel arithmetic in fp32.  x1 = the ground truth, x2 = the estimate, both (B, 3, H, W); n = 3 B H W.
 *   window: w = g (x) g with g_i = exp(-(i - 3)^2 / 4.5) / sum_j exp(-(j - 3)^2 / 4.5), i = 0 .. 6 (7 x 7 Gaussian, sigma 1.5; g itself
 *     evaluated in fp32, so its taps sum to 1 + 3.7e-8 as torch's do), applied
 *     per channel with zero padding 3: the image is zero outside, the window is NOT renormalised at the border;
 *   m1 = w * x1, m2 = w * x2, e11 = w * x1^2, e22 = w * x2^2, e12 = w * (x1 x2);  s1 = e11 - m1^2, s2 = e22 - m2^2, s12 = e12 - m1 m2;
 *   C1 = 1e-4, C2 = 9e-4;  N1 = 2 m1 m2 + C1, N2 = 2 s12 + C2, D1 = m1^2 + m2^2 + C1, D2 = s1 + s2 + C2;  S = N1 N2 / (D1 D2);
 *   mse = sum (x1 - x2)^2 / n,  ssim = sum S / n,  photo = alpha mse + beta (1 - ssim).  No clamp, no mask.
 * Gradient with respect to x2:  Bm = -S / D2,  Cm = 2 N1 / (D1 D2),  Am = 2 m1 N2 / (D1 D2) - 2 m2 S / D1 - 2 m2 Bm - m1 Cm, the three
 *   maps zero outside the image;  d(sum S) / d x2 = w * Am + 2 x2 (w * Bm) + x1 (w * Cm) (the zero-padded symmetric window is its own
 *   adjoint);  G = alpha 2 (x2 - x1) / n - (beta / n) d(sum S) / d x2.
 * Sums over pixels in fp64: one partial pair per workgroup in d_workspace, added in a fixed order by a one-workgroup launch that
 * writes the fp32 results.  No atomics: bit-identical from call to call, whatever d_workspace, d_grad and d_out3 held before.
 *
 * gdb_loss_workspace_bytes: enough for gdb_photometric_loss on (B, 3, H, W) and for gdb_smooth_l1_masked on B H W elements.
 * gdb_photometric_loss: d_est (B, 3, H, W) contiguous; d_gt read in place at element strides (gt_sb, gt_sc, gt_sy, gt_sx), none
 *   negative: (3 H W, H W, W, 1) for NCHW, (3 H W, 1, 3 W, 3) for the (B, H, W, 3) frames a data loader hands over.  d_grad (B, 3, H, W)
 *   receives G, or NULL: the adjoint half is then not run (evaluation) and d_out3 holds the same bits.  d_out3 = [mse, ssim, photo].
 * gdb_smooth_l1_masked (the monitor of train/losses/gdb_nerf.py, forward only): d_out1[0] = the mean over the elements with
 *   mask > 0.5 of smooth-L1(est - gt) with beta 1 (0.5 d^2 for |d| < 1, else |d| - 0.5); 0 / 0 = NaN for an empty mask, as the mean of
 *   an empty tensor is.  d_est, d_gt, d_mask: n contiguous floats each.
 * Refused before any launch: B, H or W < 1, n < 1, or sizes the launch grid cannot hold (GDB_E_SHAPE); a NULL required pointer, a
 * negative stride or a workspace that is too small (GDB_E_BADARG). */
int gdb_loss_workspace_bytes(int32_t B, int32_t H, int32_t W, size_t* out_bytes);
int gdb_photometric_loss(const float* d_est /* (B,3,H,W) contiguous */, const float* d_gt, int64_t gt_sb, int64_t gt_sc,
                         int64_t gt_sy, int64_t gt_sx /* element strides: NCHW or the permuted NHWC view */,
                         int32_t B, int32_t H, int32_t W, float alpha, float beta, float* d_grad /* (B,3,H,W) or NULL */,
                         void* d_workspace, size_t ws_bytes, float* d_out3 /* mse, ssim, photo */, void* stream);
int gdb_smooth_l1_masked(const float* d_est, const float* d_gt, const float* d_mask, int64_t n,
                         void* d_workspace, size_t ws_bytes, float* d_out1, void* stream);

/* ---- the depth net's train-time stage render: auxiliary NeRF + un-normalised composite, forward and backward (ABI v7, added;
 * DESIGN.md 4.18) ----------------------------------------------------------------------------------------------------------------
 * The per-stage NeRF of the reference's DepthNet (networks/gdb_nerf/depth_net.py:201-298) on materialised samples, and the composite
 * of its _render_rays (:109-114): alpha = 1 - e^-sigma, T_i = prod_{j<i} (1 - alpha_j + 1e-10), rgb_map = sum_i alpha_i T_i c_i, not
 * normalised.  The batch is folded into n_rays; ray r owns the samples [r S, (r + 1) S).
 * Accepted (anything else is refused before the first launch): feat_dim 8, 16 or 32, voxel_dim 8, hid_dim 64, viewdir_agg 0 or 1
 * (GDB_E_BADARG otherwise); 2 <= V <= GDB_MAX_VIEWS (V < 2: GDB_E_SHAPE, as gdb_mlp_backward_layout), 1 <= S <= GDB_MAX_SAMPLES,
 * V * ceil4(S) <= 64 - a tile holds whole rays and at most 64 (view, sample) rows, a view's block padded to a multiple of four
 * samples - and 1 <= n_rays < 2^31 / S (GDB_E_SHAPE otherwise).
 * gdb_stage_nerf_packed_floats / gdb_pack_stage_nerf_weights / gdb_unpack_stage_nerf_grads (host only): the packed fp32 buffer of the 16
 *   tensors view_fc.0, global_fc.0, agg_w_fc.0, fc.0, lr0.0, sigma.0, color.0, color.2 - weight then bias each, host pointers, row-major
 *   as nn.Linear stores them.  Without viewdir_agg the first two pointers are not read (not written by unpack) and view_fc's slots
 *   are zero.  Pad slots are zero.  The gradient buffer of gdb_stage_nerf_backward has the same layout.
 * gdb_stage_nerf_layout: out[0] = workspace bytes of gdb_stage_nerf_backward, out[1] = partials (workgroups) per launch, out[2] = rays
 *   per tile.
 * gdb_stage_nerf: d_vox (n_rays*S, 8); d_img (n_rays*S, V, feat_dim+3+4), the reference's sample-major layout; d_rgb_map (n_rays, 3);
 *   d_sigma (n_rays*S) and d_rgb (n_rays*S, 3) optional (NULL: not written).  One launch.
 * gdb_stage_nerf_backward: the same inputs and d_g_rgb_map (n_rays, 3) -> d_g_packed (the packed layout, overwritten), d_g_vox and
 *   d_g_img (shapes of d_vox / d_img; either may be NULL).  Nothing is saved by the forward: activations are recomputed per tile.
 *   Weight gradients accumulate in registers over a workgroup's tiles; each workgroup writes one partial to d_workspace and a second
 *   launch adds the partials in workgroup order in double: no floating-point atomics, bit-identical from run to run.  The workspace's
 *   contents on entry do not matter.  A short workspace is GDB_E_WORKSPACE, a NULL required pointer GDB_E_BADARG. */
int gdb_stage_nerf_packed_floats(int32_t feat_dim, int32_t voxel_dim, int32_t hid_dim, int32_t viewdir_agg, size_t* out_floats);
int gdb_pack_stage_nerf_weights(int32_t feat_dim, int32_t voxel_dim, int32_t hid_dim, int32_t viewdir_agg,
                                const float* const h_tensors[16], float* h_out);
int gdb_unpack_stage_nerf_grads(int32_t feat_dim, int32_t voxel_dim, int32_t hid_dim, int32_t viewdir_agg,
                                const float* h_packed, float* const h_tensors[16]);
int gdb_stage_nerf_layout(int32_t feat_dim, int32_t voxel_dim, int32_t hid_dim, int32_t viewdir_agg, int32_t V, int32_t S,
                          int64_t n_rays, size_t out[3]);
int gdb_stage_nerf(int32_t feat_dim, int32_t voxel_dim, int32_t hid_dim, int32_t viewdir_agg, const float* d_packed, int32_t V, int32_t S,
                   const float* d_vox, const float* d_img, int64_t n_rays, float* d_rgb_map, float* d_sigma, float* d_rgb, void* stream);
int gdb_stage_nerf_backward(int32_t feat_dim, int32_t voxel_dim, int32_t hid_dim, int32_t viewdir_agg, const float* d_packed, int32_t V,
                            int32_t S, const float* d_vox, const float* d_img, int64_t n_rays, const float* d_g_rgb_map, float* d_g_packed,
                            float* d_g_vox, float* d_g_img, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- the cost-regularisation U-Nets in training mode: forward with batch statistics, and backward (ABI v7, added)
 * _UNet3d.forward as the module computes it in .train(): every BatchNorm3d normalises with its batch's per-channel mean and biased
 * variance over B*D*H*W, then ReLU; running_mean / running_var move by `momentum` (the unbiased variance for running_var) and
 * num_batches_tracked grows by one, all on the device, in place.  The backward differentiates through the statistics.  Exact fp32 on
 * v_mfma_f32_16x16x4_f32; statistics and every reduction are summed in double in a fixed order: no atomics, bit-identical runs.
 * Accepted plans: those of gdb_cost_reg (depth 2 or 3, cin a multiple of 8 <= 256, base a multiple of 8 with base << depth <= 128,
 * cout 1 .. 15: GDB_E_BADARG otherwise; D, H, W divisible by 2^depth: GDB_E_SHAPE otherwise), and one refusal more: a deepest level
 * with a single value per channel (B * D*H*W >> 3 depth == 1) is GDB_E_SHAPE, as PyTorch refuses it.  Every refusal comes before the
 * first launch.
 *
 * d_params (a HOST array of DEVICE pointers), for i = 0 .. 3 depth: conv{i}.0.weight, conv{i}.1.weight, conv{i}.1.bias,
 *   conv{i}.1.running_mean, conv{i}.1.running_var, conv{i}.1.num_batches_tracked (int64) - six per layer, the last three may be NULL
 *   (not updated) and are not read by the backward - then feat_head.weight and prob_head.weight: 6 (3 depth + 1) + 2 pointers, the
 *   tensors in their own (PyTorch) layouts.  Weights are packed on the device; no parameter is copied to the host.
 * d_grads (a HOST array of DEVICE pointers): conv{i}.0.weight, conv{i}.1.weight, conv{i}.1.bias gradients - three per layer - then
 *   feat_head.weight's and prob_head.weight's: 3 (3 depth + 1) + 2 pointers, each in its tensor's own layout, overwritten.
 *
 * gdb_cost_reg_train_layout (host only, launches nothing): the named regions of the saved buffer (buffer 0) and of the backward's
 *   workspace (buffer 1) and the two byte counts; out may be NULL to query *out_count.  Saved buffer, by name (BN layer i):
 *     "conv{i}.z"       the raw convolution output, channel-last (B, D >> l, H >> l, W >> l, channels), l = level
 *     "conv{i}.out"     relu(bn(z)), and for a transposed layer skip + relu(bn(z)): what the next layer reads
 *     "conv{i}.mean", "conv{i}.invstd"   the batch mean and 1 / sqrt(biased variance + eps), `channels` floats each
 *     "prob"            the softmax output; "packed", "heads.weight", "stat_partials": the forward's own scratch.
 *   Workspace: "grad.l{l}" / "dz.l{l}" (the gradient of level l's activation and of the raw output being processed), "upstream"
 *   (B, cout + 1, D, H, W), "packed_dx", "heads.weight_bwd", "heads.weight_grad", "bn_partials", "bn_means", and the weight gradient's
 *   partials "dw_partials" (fp32, one per slab) and "dw_partials2" (double, one per 16 slabs).  Contents on entry do not matter.
 * gdb_cost_reg_train: d_cost (B, cin, D, H, W) read in place -> d_volume (B, cout, D, H, W), d_prob (B, D, H, W), and d_batch_stats
 *   (optional): per BN layer in order [mean | biased variance] x its channels.
 * gdb_cost_reg_train_backward: d_g_volume / d_g_prob are the upstream of the two outputs (either may be NULL: zero); d_cost and
 *   d_saved as the forward left them.  The gradient of d_cost is not built.  ReLU'(0) = 0.  A short buffer is GDB_E_WORKSPACE. */
typedef struct GdbCostRegTrainRegion {
    char name[32];
    uint64_t offset;    /* bytes from the start of its buffer */
    uint64_t bytes;
    int32_t buffer;     /* 0: the saved buffer, 1: the backward's workspace */
    int32_t channels;   /* 0 when the region is not per channel */
    int32_t level;      /* resolution (D, H, W) >> level, -1 when the region is not a volume */
    int32_t reserved;
} GdbCostRegTrainRegion;
int gdb_cost_reg_train_layout(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, int32_t B, int32_t D, int32_t H, int32_t W,
                              GdbCostRegTrainRegion* out, int32_t capacity, int32_t* out_count, size_t* saved_bytes, size_t* ws_bytes);
int gdb_cost_reg_train(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* d_cost, int32_t B, int32_t D,
                       int32_t H, int32_t W, const void* const* d_params, float eps, float momentum, void* d_saved, size_t saved_bytes,
                       float* d_volume, float* d_prob, float* d_batch_stats, void* stream);
int gdb_cost_reg_train_backward(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* d_cost, int32_t B, int32_t D,
                                int32_t H, int32_t W, const void* const* d_params, const float* d_g_volume, const float* d_g_prob,
                                const void* d_saved, size_t saved_bytes, void* d_workspace, size_t ws_bytes, float* const* d_grads,
                                void* stream);
/* The same backward, handing back the cost volume's gradient as well (additions to ABI v7): d_g_cost (B, cin, D, H, W),
 * planar like d_cost, = conv0's data gradient - the shared convolution body once more, stride 1, flipped taps, roles swapped, base ->
 * cin channels - out of d_cost_workspace, gdb_cost_reg_train_cost_grad_bytes bytes of scratch of its own (conv0's repacked weights and
 * the gradient channel-last; contents on entry do not matter; a short one is GDB_E_WORKSPACE, a NULL one GDB_E_BADARG).  With
 * d_g_cost == NULL the scratch is not read and the work and the results are those of gdb_cost_reg_train_backward, bit for bit; with
 * it, the parameter gradients are those same bits.  gdb_cost_reg_train_layout answers as before. */
int gdb_cost_reg_train_cost_grad_bytes(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, int32_t B, int32_t D, int32_t H,
                                       int32_t W, size_t* out_bytes);
int gdb_cost_reg_train_backward_cost(int32_t depth, int32_t cin, int32_t base_channels, int32_t cout, const float* d_cost, int32_t B,
                                     int32_t D, int32_t H, int32_t W, const void* const* d_params, const float* d_g_volume,
                                     const float* d_g_prob, const void* d_saved, size_t saved_bytes, void* d_workspace, size_t ws_bytes,
                                     float* const* d_grads, float* d_g_cost, void* d_cost_workspace, size_t cost_ws_bytes, void* stream);

/* ---- the optimiser step: clip_grad_value_ + Adam / AdamW over n fp32 tensors in one call (addition to ABI v7)
 * Every array argument is a HOST array with one entry per tensor: the four DEVICE pointers (parameter, gradient, exp_avg, exp_avg_sq,
 * each numel[i] contiguous floats, 4-byte aligned at least; the four may not overlap), the element count, the tensor's own
 * hyper-parameters as doubles, and its own step count t = step[i], ALREADY incremented (the first step passes 1).  clip_value <= 0
 * means no clipping; decoupled != 0 is AdamW.  Per tensor the host forms, in double, 1 - beta1, 1 - beta2, 1 - lr weight_decay,
 * step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) and rounds each to float once - what torch's single-tensor Adam does
 * with a Python-number step.  Per element, in this order, each step one fp32 rounding (no fused multiply-add):
 *   1. clip_value > 0:  g = g < -c ? -c : (g > c ? c : g), and the clamped value is WRITTEN BACK to the gradient, as clip_grad_value_
 *      leaves it.  A NaN gradient stays NaN (torch.clamp), +-inf becomes +-c.  Without clipping the gradient is only read.
 *   2. weight_decay != 0:  Adam (L2): g' = g + wd p (the stored gradient keeps the clamped g);  AdamW: p = p (1 - lr wd).
 *   3. m = m + (g' - m)(1 - beta1);   v = v beta2;   v = v + (1 - beta2) g' g'.
 *   4. denom = sqrt(v) / bc2_sqrt + eps;   p = p - step_size (m / denom).
 * ceil(tensors / 48) launches on `stream`, each taking its tensors' pointers by value in the kernel arguments: no device-resident
 * table, no workspace, no host synchronisation, no process-global state.  Every element is owned by one lane: two calls from the
 * same state give the same bits.  Tensors with numel 0 take no part; n == 0 or all numel 0 is GDB_OK with no launch.
 * Refused before anything is launched: n < 0, a NULL array, a NULL pointer among a tensor's four, step < 1, a beta outside [0, 1)
 * (GDB_E_BADARG); numel < 0 or beyond 2^31 - 1 chunks of 2048 elements (GDB_E_SHAPE). */
int gdb_adam_step(int32_t n, float* const* d_param, float* const* d_grad, float* const* d_exp_avg, float* const* d_exp_avg_sq,
                  const int64_t* numel, const double* lr, const double* beta1, const double* beta2, const double* eps,
                  const double* weight_decay, const int64_t* step, double clip_value, int32_t decoupled, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GDB_NERF_HIP_H */
