/*
 * arah_hip.h -- C ABI of the MI355X (gfx950) implementation of ARAH's articulated-SDF
 * volume-rendering hot path.
 *
 * The reference (taconite/arah-release) is pure Python: there is no FFI in it.  The interfaces
 * these entry points replace are the Python seams of the hot path (paths relative to the
 * reference root):
 *
 *   arah_trace              BodyRayTracing.sphere_tracing + search_iso_surface_depth
 *                           im2mesh/metaavatar_render/renderer/ray_tracing.py:174-296,
 *                           im2mesh/utils/root_finding_utils.py:365-484
 *   arah_sample_canonicalize BodyRayTracing.ray_sampler / inv_transform_points_opt /
 *                           search_canonical_corr  ray_tracing.py:313-461, root_finding_utils.py:267-362
 *   arah_shade_composite    IDHRNetwork.get_rbg_value_vol_sdf + the eval tail of forward
 *   arah_shade_points       its per-sample half (SDF, normal, colour, density) on the shipped engine
 *                           renderer/implicit_differentiable_renderer.py:261-396, :142-148,:225-257
 *   arah_render             IDHRNetwork.forward (eval)  implicit_differentiable_renderer.py:42-259
 *   arah_render_maps        arah_render + the composited normal and depth maps (no reference counterpart: the VolSDF
 *                           compositing of the posed SDF normal, implicit_differentiable_renderer.py:338-340, 370-394)
 *   arah_sdf_eval           sdf_network(x) / gradient(sdf, x)   hyperlayers.py:385-415,
 *                           siren_modules.py:35-37, diff_operators.py:39-50
 *   arah_skin_lbs           forward_skinning / query_weights  root_finding_utils.py:54-167,
 *                           utils/utils.py:138-181, metaavatar/models/decoder.py:201-233
 *   arah_skin_jacobian      forward_skinning_jac  root_finding_utils.py:170-226
 *   arah_color_eval         RenderingNetwork.forward  metaavatar_render/models/decoder.py:69-124
 *   arah_nearest_inverse_lbs inv_transform_points_smpl_verts  ray_tracing.py:382-400
 *                           (pytorch3d.ops.knn_points K=1 + nearest-vertex inverse LBS)
 *   arah_broyden3_lbs       search_canonical_corr on caller-supplied initial guesses
 *                           (broyden.py:4-78 with g = LBS(x) - target)
 *   arah_joint_root_find    search_iso_surface_depth on caller-supplied starts  root_finding_utils.py:365-484
 *   arah_sdf_grid           create_mesh_vertices_and_faces' lattice evaluation  utils/sdf_meshing.py:13-70
 *   arah_marching_cubes     skimage.measure.marching_cubes_lewiner as called at utils/sdf_meshing.py:95 (+ :96-101)
 *   arah_marching_cubes_indexed   the same call's (verts, faces) result, utils/sdf_meshing.py:95-114: shared vertices
 *   arah_mesh_components /  (none: the reference writes the extracted mesh as it comes; connected components of an indexed mesh
 *   arah_mesh_select        by shared vertex ids, and the order-preserving selection of some of them: floater removal)
 *   arah_mesh_simplify      (none: vertex clustering of an indexed mesh on a grid: decimation and welding by position)
 *   arah_mesh_quadric_place (none: the clusters of arah_mesh_simplify moved to the minimisers of their faces' plane quadrics)
 *   arah_mesh_collapse_round (none: one round of edge-collapse decimation that keeps the surface a surface)
 *   arah_mesh_subdivide_round (none: one round of midpoint or Loop subdivision, of every edge or of the long ones)
 *   arah_mesh_flip_round    (none: one round of independent edge flips, towards Delaunay or towards valence six)
 *   arah_mesh_adjacency /   (none: the reference's users smooth and re-normal with trimesh / open3d / pytorch3d; the incident faces
 *   arah_mesh_vertex_normals /  and unique neighbours of every vertex with edge statistics, pytorch3d's verts_normals_packed over
 *   arah_mesh_smooth        them, and Laplacian / Taubin umbrella smoothing)
 *   arah_mesh_cotangent /   (none: the cotangent Laplacian of an indexed mesh with its lumped mass and angle sums, the operator applied
 *   arah_mesh_laplacian_apply /  to per-vertex values, mean / Gaussian / principal curvatures after Meyer, Desbrun, Schroeder and Barr
 *   arah_mesh_curvature /   2002, and umbrella smoothing with cotangent weights: what the reference's users take from trimesh, libigl
 *   arah_mesh_smooth_cotangent   or pytorch3d)
 *   arah_mesh_solve_begin / (none: systems with that operator by preconditioned conjugate gradients -- implicit smoothing, harmonic
 *   arah_mesh_solve_steps   extension; what the reference's users take from scipy's or libigl's sparse solvers)
 *   arah_mesh_orient /      (none: the reference's users repair scans with trimesh's fix_normals / fill_holes; consistent orientation
 *   arah_mesh_boundary_loops /  by the double cover of the face graph, the boundary loops, and small holes closed by a fan around
 *   arah_mesh_fill_holes    the loop's exact mean)
 *   arah_mesh_intersections (none: the pairs of faces that cut through each other, by an exact integer predicate on the lattice of
 *                           arah_mesh_orient; with a group label, the intersections between two meshes)
 *   arah_mesh_rasterize /   pytorch3d MeshRasterizer's three outputs for an INDEXED mesh (pix_to_face, zbuf, bary_coords; one face per
 *   arah_mesh_interpolate   pixel, no blur, perspective-correct) and interpolate_face_attributes over them; arah_rasterize below
 *                           stays what the gen_cano_mesh branch draws with
 *   arah_rasterize          pytorch3d MeshRasterizer (pix_to_face) as used at metaavatar_render/models/__init__.py:232-276
 *   arah_shade_train_*      get_rbg_value_vol_sdf with self.training: per-sample forward and backward
 *                           renderer/implicit_differentiable_renderer.py:291-361, diff_operators.py:39-50
 *   arah_gram_skinny        the matmul backward of autograd for the 1- / 3-row heads and the K = 3 first layer
 *                           (weight gradients summed over ~1e5 samples)
 *   arah_query_posed        inv_transform_points_opt + the SDF evaluation of the depth samples, on arbitrary posed points
 *                           ray_tracing.py:403-461, implicit_differentiable_renderer.py:336-359
 *   arah_sdf_grid_posed     the same on a lattice of posed space (no reference counterpart: the reference meshes the canonical
 *                           lattice only and skins that mesh forward, models/__init__.py:209-227)
 *   arah_image_metrics      psnr_metric / ssim_metric of a validation frame  im2mesh/utils/eval.py:6-18
 *                           (skimage.metrics.structural_similarity + cv2.boundingRect; called at lightning_model.py:216-224)
 *   arah_mesh_closest /     (none: geometry scores of posed meshes against ground-truth meshes; the reference's README points
 *   arah_surface_metrics    to a script outside its tree)
 *   arah_mesh_query         check_mesh_contains + igl.point_mesh_squared_distance + igl.barycentric_coordinates_tri
 *                           im2mesh/utils/libmesh/inside_mesh.py:4-160, im2mesh/data/zju_mocap.py:466-529
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name starts with "h_"; the caller owns all
 *     buffers, including the workspace; nothing is allocated, freed or synchronised inside;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); calls are re-entrant
 *     across streams as long as workspaces differ;
 *   - return value: 0 on success, negative ARAH_E_* on error; nothing throws;
 *   - floats are IEEE fp32, masks are uint8 (0/1), indices int32; arrays are dense row-major.
 */
#ifndef ARAH_HIP_H
#define ARAH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARAH_OK 0
#define ARAH_E_BADARG (-1)      /* null pointer / negative size */
#define ARAH_E_SHAPE (-2)       /* network shape not supported by the compiled kernels */
#define ARAH_E_WORKSPACE (-3)   /* workspace or frame buffer too small */
#define ARAH_E_LAUNCH (-4)      /* HIP launch error (hipGetLastError) */
#define ARAH_E_SAMPLING (-5)    /* n_steps < n_near + n_far + 1, or n_steps > ARAH_MAX_STEPS */
#define ARAH_E_OVERFLOW (-6)    /* a data-dependent count does not fit an int32 */

#define ARAH_MAX_STEPS 128
#define ARAH_N_JOINTS 24
#define ARAH_COLOR_NO_VIEW_DIR 0 /* input [x, n, feat, pose]         (ZJUMOCAP-377-mono) */
#define ARAH_COLOR_IDR 1         /* input [x, PE4(view), n, feat, pose] (ZJUMOCAP-313, H36M) */

/* GEMM engine of the forward SDF trunks (every result stays fp32-class, see csrc/mlp.hpp):
 *   SPLIT_F16: fp32 operands carried as hi + lo f16 pairs, three v_mfma_f32_16x16x32_f16 per product, fp32
 *              accumulation (22 significant bits per operand; error vs fp64 at or below the exact engine's);
 *   FP32     : v_mfma_f32_16x16x4_f32 everywhere (bit-for-bit an fmaf chain), 16/3 x the matrix-pipe time. */
#define ARAH_PRECISION_SPLIT_F16 0
#define ARAH_PRECISION_FP32 1

/* Row-major, un-packed network weights as PyTorch holds them (weight-norm already folded:
 * W = g * v / |v|).  Shapes are the ones every ARAH config uses; arah_prepare_frame rejects
 * anything else with ARAH_E_SHAPE. */
typedef struct ArahNets {
    /* emitted FiLM-SIREN SDF MLP 3 -> 256 x6 -> 1  (hyperlayers.py:497-510) */
    const float* sdf_w[7];      /* [256,3], 5 x [256,256], [1,256] */
    const float* sdf_b[7];      /* [256] x6, [1] */
    const float* film_freq;     /* [6*256] */
    const float* film_phase;    /* [6*256] */
    /* skinning MLP 3 -> 128 x4 -> 25, Softplus(beta=100) */
    const float* skin_w[5];     /* [128,3], 3 x [128,128], [25,128] */
    const float* skin_b[5];
    /* colour MLP in -> 256 -> 256 -> 128 -> (in+128) -> 256 -> 256 -> 3, ReLU, sigmoid, skip at 3 */
    const float* col_w[6];      /* [256,in], [256,256], [128,256], [256,in+128], [256,256], [3,256] */
    const float* col_b[6];
    const float* pose_vec;      /* [n_pose] per-frame constant tail of the colour input (may be NULL if n_pose==0) */
    int32_t col_mode;           /* ARAH_COLOR_* */
    int32_t n_pose;             /* 128 for color_pose_encoder 'latent' */
    const float* beta;          /* [1] DEVICE: |variance|, un-clipped (NULL: 1e-3, the reference's initial value) */
    int32_t precision;          /* ARAH_PRECISION_* */
} ArahNets;

/* Per-frame body (lightning_model.py:581-632 keys smpl_verts, skinning_weights, bone_transforms,
 * trans, coord_min, coord_max, center), batch element 0. */
typedef struct ArahBody {
    const float* verts;         /* [n_verts,3] posed + trans */
    const float* vert_weights;  /* [n_verts,24] */
    const float* bones;         /* [24,4,4] */
    /* the four per-frame scalars are DEVICE pointers too: they are inputs of the forward (dataset tensors) and are
     * consumed by the kernels only, so that building a frame needs no device->host copy and no stream drain */
    const float* trans;         /* [3] */
    const float* center;        /* [3] */
    const float* coord_min;     /* [1] */
    const float* coord_max;     /* [1] */
    int32_t n_verts;            /* <= 6912 */
    const void* prepared;       /* NULL, or a buffer filled by arah_prepare_body for these verts: arah_prepare_frame then
                                   skips the nearest-vertex tables (its kernels read them from here; keep it alive with the
                                   frame, and order the stream that built it before the frame's stream) */
} ArahBody;

/* ArahSampling.full_shading.  The shading cull of ARAH_SHADING_LAZY (ignored by arah_render_maps): deep behind the surface
 * w = alpha * trans falls below half an ulp of the accumulated colour and r += c * w returns r for every c in [0, 1]; such
 * samples are guessed from the densities, left unshaded, and the guess is verified by the compositing walk on its own
 * accumulators (a ray that fails has them shaded after all and is composited again, on the device).  The switch is a value of
 * this field and the cull's two counters have a reader of their own (arah_shade_cull_counters), so that ArahSampling and
 * ArahCounters keep their sizes. */
enum { ARAH_SHADING_LAZY = 0, ARAH_SHADING_FULL = 1, ARAH_SHADING_LAZY_NO_CULL = 2 };
enum { ARAH_SHADE_ENGINE_DEFAULT = 0 /* bf16 x 3 on split frames */, ARAH_SHADE_ENGINE_FP32 = 1 };
enum { ARAH_CANON_KERNEL_WAVE = 0 /* point-owning waves, hi fragments in LDS */, ARAH_CANON_KERNEL_TILE = 1,
       ARAH_CANON_KERNEL_WAVE_L2 = 2 };

typedef struct ArahSampling {
    int32_t n_steps, n_near, n_far;   /* configs/default.yaml:49-51 */
    int32_t cano_view_dirs;           /* model.cano_view_dirs */
    int32_t render_last_pt;           /* model.render_last_pt */
    int32_t full_shading;             /* ARAH_SHADING_*.  0 (default): exact lazy shading -- normal + colour only for
                                         samples whose density is > 0 (the rest provably get weight 0), and of those only
                                         for the ones whose weight can still change a pixel (the shading cull, below);
                                         1: shade every valid sample like the reference does; 2: lazy shading without
                                         the cull, every sigma > 0 sample shaded.  Same image bit for bit in all three. */
    /* device copies of torch.linspace(0, 1, k) for k = n_steps, n_near + 1, n_far (RT:317,330,340);
     * the caller builds them once per config so that depth samples are bit-identical to torch's */
    const float* lin_steps;
    const float* lin_near;
    const float* lin_far;             /* may be NULL when n_far == 0 */
    /* Per-call switches and profiling hooks (round 4: they were environment variables read into process-wide statics and
     * process-wide event setters; the library now keeps no state between calls, so calls on different streams with different
     * ArahSampling objects do not see each other). */
    int32_t shade_engine;             /* ARAH_SHADE_ENGINE_*: loop D's normal sweep + colour MLP on a split-engine frame */
    int32_t canon_kernel;             /* ARAH_CANON_KERNEL_*: loop C's solver on a split-engine frame */
    /* pairs of hipEvent_t (start, stop), both non-NULL to take effect: recorded on the call's stream immediately before /
     * after the launch of loop C's solver, of the density pre-pass and of the shading kernel */
    void* ev_canon[2];
    void* ev_density[2];
    void* ev_shade[2];
    /* Tiered evaluation (round 6, csrc/tier.hpp; arah_render with full_shading == 0 only): the occupancy buffer that
     * arah_prepare_occupancy filled for THIS frame, or NULL = every sample of every ray through loops C and D like the reference
     * (ray_tracing.py:313-380, implicit_differentiable_renderer.py:261-396).  With it, samples outside the posed fat body are
     * certified sigma = +0 without being evaluated; images and masks are the untiered path's bit for bit. */
    const void* occupancy;
    /* the tiered path launches loop C's solver and the density pass twice (phase 1 / phase 2): event pairs of the second launches */
    void* ev_canon2[2];
    void* ev_density2[2];
} ArahSampling;

/* Opaque-ish handle filled by arah_prepare_frame: device pointers into the caller's frame
 * buffer (MFMA-packed weights, padded vertices) plus scalars.  POD, copy freely. */
typedef struct ArahFrame {
    const float* sdf_w0;        /* [256][4] */
    const float* sdf_wp[5];     /* packed fwd */
    const float* sdf_wpT[5];    /* packed transposed (reverse sweep) */
    const float* sdf_w6;        /* [256] */
    const float* sdf_b6;        /* [1] */
    const float* sdf_bias;      /* [6][256] */
    const float* sdf_freq;      /* [6][256] */
    const float* sdf_phase;     /* [6][256] */
    const void* sdf_wps[5];     /* split-packed fwd: hi/lo f16 planes, pre-scaled by a power of two per layer */
    const float* sdf_fw;        /* [6][256] 30 f / pi */
    const float* sdf_pw;        /* [6][256] 30 (f b + phi) / pi */
    const float* sdf_fws;       /* [6][256] fw divided by the split scales of the producing layer */
    const float* skin_w0;       /* [128][4] */
    const float* skin_wp[3];    /* packed 128x128 */
    const float* skin_w4p;      /* packed [32][128] */
    const float* skin_bias;     /* [4][128] + [32] */
    const void* skin_wps[4];    /* split-packed 128x128 x3 and [32][128] */
    const float* skin_scales;   /* [8] activation scales S_k (probed per frame) and accumulator un-scales */
    const void* skin_wpr;       /* 4 layers, split-packed in the channel order of the point-owning-wave kernels (csrc/canon_wave.hpp) */
    const float* skin_wconsts;  /* their constants: first layer, biases in z = 100 log2(e) x units, un-scales */
    const float* col_w0p;       /* packed [256][KIN_PAD] (columns permuted to [feat,x,n,view]) */
    const float* col_w1p;       /* packed [256][256] */
    const float* col_w2p;       /* packed [128][256] */
    const float* col_w3ap;      /* packed [256][KIN_PAD] */
    const float* col_w3bp;      /* packed [256][128] */
    const float* col_w4p;       /* packed [256][256] */
    const float* col_w5;        /* [3][256] */
    const float* col_bias;      /* b0'[256] b1[256] b2[128] b3'[256] b4[256] b5[4] */
    const float* col_w0pT;      /* transposed packings of the colour MLP (reverse sweep of the training backward) */
    const float* col_w1pT;
    const float* col_w2pT;
    const float* col_w3apT;
    const float* col_w3bpT;
    const float* col_w4pT;
    const void* b3[22];         /* bf16 hi/lo fragments of the SDF (W, W^T) and colour (W, W^T) matrices: operands of the
                                   training kernels' bf16 x 3 products (arah_shade_train_forward / _backward) */
    const float* verts4;        /* [256][28][4] k-d clustered vertices (x, y, z, original index) */
    const float* knn_spheres;   /* [256][4] bounding spheres of the clusters */
    const void* knn_grid;       /* grid geometry (device) */
    const void* knn_cells;      /* [n_cells][64] candidate clusters per cell */
    const float* verts;         /* caller's [n_verts][3] */
    const float* vert_T;        /* [n_verts][16] blended bone transform of each vertex, sum_j w_vj A_j (frame buffer) */
    const float* bones;         /* caller's [24][16] */
    const float* scalars;       /* [9] device: trans(3), center(3), coord_min, coord_max, |variance| */
    int32_t n_verts;
    int32_t col_mode;
    int32_t precision;          /* ARAH_PRECISION_* the frame was prepared for */
} ArahFrame;

/* Work counters (points evaluated), SURVEY 8(d). */
typedef struct ArahCounters {
    uint64_t n_sdf_fwd, n_sdf_grad, n_skin_fwd, n_skin_jac, n_col, n_knn;
    uint64_t n_density;   /* samples seen by the density pre-pass of lazy shading (a subset of n_sdf_fwd) */
    uint64_t n_canon;     /* skinning-MLP evaluations of loop C (k_canon_wave / k_canon_solve; a subset of n_skin_fwd) */
    uint64_t n_split_nonfinite; /* loop-C evaluations of the split engine whose residual was not finite (an activation
                                   left the f16 range): non-zero means the frame should be re-prepared with
                                   ARAH_PRECISION_FP32 */
    /* tiered eval forward: rays classified; of them surface rays (loops A+B converged), promoted to the exact tier, skipped
     * (certified rgb = 0); samples evaluated in phase 1 (surface rays, marked samples, witnesses), in phase 2 (the rest of the
     * promoted rays), never evaluated; rays that sent a witness */
    uint64_t n_tier_rays, n_tier_rays_surface, n_tier_rays_promoted, n_tier_rays_skipped;
    uint64_t n_tier_samples_p1, n_tier_samples_p2, n_tier_samples_skipped, n_tier_witnesses;
    uint64_t n_tier_rays_untraced;       /* rays whose [near, far] segment misses the posed fat body: loops A+B not run */
    uint64_t n_canon_p2, n_density_p2;   /* the share of n_canon / n_density that phase 2 ran */
} ArahCounters;

/* ---- frame preparation ------------------------------------------------------------------ */
/* Optional early half: the nearest-vertex tables of a posed body (what ray_tracing.py:382-400 asks pytorch3d's
 * knn_points for, per call) depend on the vertices only.  arah_prepare_body builds them into a caller buffer of
 * arah_body_bytes() bytes (256-byte aligned) on `stream` -- typically a side stream, while the caller's stream runs the
 * pose encoder and the hypernetwork; pass the buffer as ArahBody.prepared to arah_prepare_frame. */
size_t arah_body_bytes(void);
int arah_prepare_body(const float* verts, int32_t n_verts, void* body_buf, size_t body_bytes, void* stream);
size_t arah_frame_bytes(const ArahNets* h_nets, const ArahBody* h_body);
int arah_prepare_frame(const ArahNets* h_nets, const ArahBody* h_body, void* frame_buf, size_t frame_bytes,
                       ArahFrame* h_frame_out, void* stream);

/* ---- workspace -------------------------------------------------------------------------- */
size_t arah_workspace_bytes(int32_t n_rays, int32_t n_steps);
/* zero / read the device-side work counters that live at the head of a workspace */
int arah_counters_reset(void* workspace, void* stream);
int arah_counters_read(const void* workspace, ArahCounters* h_out, void* stream); /* syncs the stream */
/* The shading cull's two counters, which sit in the workspace directly behind ArahCounters (arah_counters_reset zeroes them
 * too): h_out2[0] = n_shade_culled, sigma > 0 samples never shaded; h_out2[1] = n_shade_rescued, samples set aside first
 * and shaded after all because their ray failed the check.  n_col keeps counting what was shaded:
 * n_col + n_shade_culled = sigma > 0 samples.  Syncs the stream. */
int arah_shade_cull_counters(const void* workspace, uint64_t* h_out2, void* stream);

/* ---- unit seams (parity tests; also usable on their own) --------------------------------- */
/* n_pts = 0 is accepted by every seam: nothing is read or written, and the point / output pointers may be null */
/* x_norm [P,3] -> sdf [P] (normalised units), optional feat [P,256], optional grad [P,3] */
int arah_sdf_eval(const ArahFrame* h_frame, const float* x_norm, int32_t n_pts, float* sdf, float* feat,
                  float* grad, void* workspace, size_t workspace_bytes, void* stream);
/* SDF on the N^3 lattice of [-1,1]^3 (utils/sdf_meshing.py:13-70): sdf[(ix*N + iy)*N + iz], normalised units */
int arah_sdf_grid(const ArahFrame* h_frame, int32_t n_side, float* sdf, void* workspace, size_t workspace_bytes,
                  void* stream);
/* The same lattice for marching cubes at level 0 (utils/sdf_meshing.py:95 only reads the corners of cells that change sign):
 * exact values wherever the level set can pass -- coarse cells (1/32 of the box) whose corner values and own slope admit a zero,
 * plus their 26 neighbours -- and a value of the right sign elsewhere.  list: [N^3] int32 scratch; scratch:
 * arah_sdf_grid_band_scratch_bytes() bytes.  Same triangle soup as arah_sdf_grid + arah_marching_cubes; N >= 33. */
size_t arah_sdf_grid_band_scratch_bytes(void);
int arah_sdf_grid_band(const ArahFrame* h_frame, int32_t n_side, float* sdf, int32_t* list, void* scratch,
                       size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* nearest covering face per pixel (pix_to_face of the rasteriser models/__init__.py:232-237 uses): tri [F,3,3] =
 * (u, v, z) per corner in pixel coordinates / view depth; zbuf [H*W] keys (depth bits << 32 | face), pre-set to ~0 */
int arah_rasterize(const float* tri_uvz, int32_t n_faces, int32_t height, int32_t width, float z_near,
                   uint64_t* zbuf, void* stream);
/* raw canonical x_hat [P,3] -> optional w [P,24], x_bar [P,3], T [P,16] */
int arah_skin_lbs(const ArahFrame* h_frame, const float* x_hat, int32_t n_pts, float* w, float* x_bar,
                  float* T, void* workspace, size_t workspace_bytes, void* stream);
/* arah_skin_lbs for a point list whose length is known on the DEVICE only: the first min(n_max, *n_items * per_item) rows
 * of x_hat are skinned into x_bar, the other rows of x_bar are left as the caller set them.  (The vertices of the mesh
 * arah_marching_cubes just extracted: per_item = 3 corners per triangle; no host round trip for the count.) */
int arah_skin_lbs_counted(const ArahFrame* h_frame, const float* x_hat, int32_t n_max, const int32_t* n_items,
                          int32_t per_item, float* x_bar, void* workspace, size_t workspace_bytes, void* stream);
/* Level set of a lattice volume as a triangle soup (the call utils/sdf_meshing.py:95 makes to
 * skimage.measure.marching_cubes_lewiner, followed by :96-101's vertex = origin + index * voxel_size on the lattice of
 * [-1,1]^3).  sdf [n][n][n] indexed [ix][iy][iz]; tri_table [256][16] int8 / n_tri [256] int32 (DEVICE): for every
 * inside-outside pattern of a cell's 8 corners (bit c set = corner c below `level`; corner / edge numbering of
 * arah_release_amd/meshing.py) the edge ids of its triangles, -1 padded, and their number (<= 5).  -> tris [cap][3][3]
 * coordinates in [-1,1]^3, right-hand normals towards decreasing values, cells in (ix, iy, iz) order; rows beyond the count
 * are ZERO (degenerate triangles); *n_tris (device) = the number of triangles of the level set, which may exceed cap (then
 * only the first cap were written).  Shared vertices of neighbouring cells are bit-equal.  scratch:
 * arah_marching_cubes_scratch_bytes(n_side) device bytes.  No host synchronisation. */
size_t arah_marching_cubes_scratch_bytes(int32_t n_side);
int arah_marching_cubes(const float* sdf, int32_t n_side, float level, const int8_t* tri_table, const int32_t* n_tri,
                        float* tris, int32_t cap, int32_t* n_tris, void* scratch, size_t scratch_bytes, void* stream);
/* The same level set as an INDEXED mesh (the (verts, faces) pair utils/sdf_meshing.py:13-114 returns): one vertex per
 * crossing lattice edge.  The edge that leaves point (ix, iy, iz) along axis a (0 x, 1 y, 2 z; a point on the last layer of
 * an axis has no edge along it) has the key ((ix n + iy) n + iz) 3 + a and crosses when (sdf[lo] < level) != (sdf[hi] < level).
 * -> verts [vert_cap][3]: the crossing edges in ascending key order, each bit-equal to every corner arah_marching_cubes puts
 * on that edge; vert_edge [vert_cap] (may be NULL): their keys; faces [face_cap][3]: triangle f of arah_marching_cubes on the
 * same volume, corner for corner (after its orientation flip), as vertex ids; counts (device int32[2]) = the number of
 * vertices and of faces of the level set, which may exceed the caps (then only the first vert_cap vertices and the first
 * face_cap faces were written, and a written face may name a vertex beyond vert_cap).  Rows between a count and its cap are
 * ZERO.  n_side >= 2 and 3 n^3 <= INT32_MAX (n <= 894); scratch: arah_marching_cubes_indexed_scratch_bytes(n_side) device
 * bytes (0 for an n_side out of range).  Deterministic: no atomics.  No host synchronisation. */
size_t arah_marching_cubes_indexed_scratch_bytes(int32_t n_side);
int arah_marching_cubes_indexed(const float* sdf, int32_t n_side, float level, const int8_t* tri_table, const int32_t* n_tri,
                                float* verts, int32_t vert_cap, int32_t* vert_edge, int32_t* faces, int32_t face_cap,
                                int32_t* counts, void* scratch, size_t scratch_bytes, void* stream);
/* Connected components of an indexed mesh.  faces [n_faces][3] vertex ids; two vertices are connected when a face names both
 * (positions play no part).  A face with an id outside [0, n_verts) is SKIPPED (a truncated arah_marching_cubes_indexed may
 * name a vertex beyond vert_cap); a vertex no valid face names is a component of its own with 0 faces.  -> labels [n_verts]:
 * the component of every vertex, dense ids in [0, C), components numbered in ascending order of their smallest vertex id;
 * comp_verts / comp_faces [n_verts]: vertices and valid faces of component c, ZERO for c >= C; counts (device int32[3]) = C,
 * the number of valid faces, the component with the most faces (ties: the lowest id; -1 when C = 0).  Integer atomics only
 * (min, add, max): the result is unique.  0 <= n_verts, n_faces <= INT32_MAX, otherwise ARAH_E_BADARG without a launch and
 * a scratch size of 0; scratch: arah_mesh_components_scratch_bytes(n_verts, n_faces) device bytes, 8-byte aligned.  Empty
 * inputs still write counts; pointers of empty arrays may be NULL.  No host synchronisation, no allocation. */
size_t arah_mesh_components_scratch_bytes(int64_t n_verts, int64_t n_faces);
int arah_mesh_components(const int32_t* faces, int64_t n_faces, int64_t n_verts, int32_t* labels, int32_t* comp_verts,
                         int32_t* comp_faces, int32_t* counts, void* scratch, size_t scratch_bytes, void* stream);
/* Order-preserving selection of components.  labels [n_verts] as above, keep [n_verts] int32 indexed by COMPONENT id.  A vertex
 * is kept when keep[labels[v]] != 0 (a label outside [0, n_verts) keeps nothing); a face is kept when its ids are valid and
 * its three vertices are kept.  -> vert_src [n_verts]: the old id of new vertex j, kept vertices in their original order;
 * vert_map [n_verts]: the new id of old vertex v, or -1; faces_out [n_faces][3]: the kept faces in their original order with
 * the new ids; face_src [n_faces]: their old rows; counts (device int32[2]) = kept vertices, kept faces.  Rows between a count
 * and the array's length are ZERO (vert_map has none).  The outputs are sized by the inputs: nothing can be truncated.  Sizes,
 * errors, scratch (arah_mesh_select_scratch_bytes) and empty inputs as for arah_mesh_components. */
size_t arah_mesh_select_scratch_bytes(int64_t n_verts, int64_t n_faces);
int arah_mesh_select(const int32_t* faces, int64_t n_faces, int64_t n_verts, const int32_t* labels, const int32_t* keep,
                     int32_t* vert_src, int32_t* vert_map, int32_t* faces_out, int32_t* face_src, int32_t* counts, void* scratch,
                     size_t scratch_bytes, void* stream);
/* Simplification of an indexed mesh by vertex clustering on a grid (csrc/meshsimp.hpp).  verts [n_verts][3], faces [n_faces][3]
 * vertex ids; the grid: h_origin (HOST float[3], finite), cell > 0 with a finite float32 reciprocal, h_dims (HOST int32[3], each
 * >= 1, at most 2^27 cells in all).  Cell of a vertex, in float32: c = clamp(floor((v - origin) (1 / cell)), 0, dims - 1) per
 * axis, key = cx + nx (cy + ny cz); a vertex with a non-finite coordinate is invalid.  The clusters are the occupied cells in
 * ascending key.  Mean of a cluster: the exact integer sum of llrint(clamp((double(v) - double(origin)) fix_scale, -2^36, 2^36))
 * over its members, divided by their number and by fix_scale, plus origin, rounded to float32; fix_scale is a power of two,
 * 2^(36 - ceil(log2(max(dims) cell))).  Representative: the member with the smallest float32 squared distance to the mean
 * (evaluated in double, one rounding per operation), ties to the lowest id.  -> verts_out [n_verts][3]: the means (position 0) or
 * the representatives' coordinates (position 1); vert_src [n_verts]: the representatives; vert_map [n_verts]: the cluster of
 * every vertex, or -1; faces_out [n_faces][3], face_src [n_faces]: the faces that survive, as cluster ids and old rows, in their
 * original order and orientation; counts (device int32[6]) = clusters K, kept faces, faces with an id outside [0, n_verts) or an
 * invalid vertex, faces collapsed (two of the three clusters equal), duplicates (dedup != 0: an earlier surviving face names the
 * same three clusters in any order), status.  Status 1: dedup with K > 2^21 (the ids do not fit the 64-bit key of a face): no
 * face is kept and none counted as a duplicate.  Rows between a count and the array's length are ZERO (vert_map has none).
 * Integer atomics only: the result is unique.  n_verts <= 2^26, n_faces <= 2^28, otherwise ARAH_E_BADARG without a launch, as
 * for any other argument out of range, and a scratch size of 0; scratch: arah_mesh_simplify_scratch_bytes(n_verts, n_faces,
 * n_cells) device bytes, 256-byte aligned.  Empty inputs still write counts; pointers of empty arrays may be NULL.  No host
 * synchronisation, no allocation. */
size_t arah_mesh_simplify_scratch_bytes(int64_t n_verts, int64_t n_faces, int64_t n_cells);
int arah_mesh_simplify(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float h_origin[3], float cell,
                       const int32_t h_dims[3], double fix_scale, int32_t position, int32_t dedup, float* verts_out,
                       int32_t* vert_src, int32_t* vert_map, int32_t* faces_out, int32_t* face_src, int32_t* counts, void* scratch,
                       size_t scratch_bytes, void* stream);
/* Quadric-error placement of the clusters of arah_mesh_simplify (csrc/meshquadric.hpp).  verts [n_verts][3], faces [n_faces][3]
 * vertex ids, vert_map [n_verts] and means [n_verts][3] (verts_out at position 0) of arah_mesh_simplify, counts its counts on the
 * DEVICE: K = counts[0] is read there, clamped to [0, n_verts].  A face is valid when its ids lie in [0, n_verts) and vert_map in
 * [0, K) for all three (a repeated id is fine); it contributes once to each distinct cluster of its corners, collapsed and
 * duplicate faces too.  In float64, every operation rounded on its own, no square root: with m = double(means[k]), pa = double(a)
 * - m (pb, pc likewise), n = (pb - pa) x (pc - pa), d = -((n0 pa0 + n1 pa1) + n2 pa2), the term of the face is A = n n^T (six
 * numbers) and b = n d.  The terms of a cluster, in ascending face id, are summed by the in-place tree "stride = 1, 2, 4, ... <
 * n: x[i] += x[i + stride] for i a multiple of 2 stride with i + stride < n".  t = (A00 + A11) + A22, M = A + (reg t) I, C the
 * cofactors of M, det = (M00 C00 + M01 C01) + M02 C02, y = -(C b) / det row by row; pos_out[k] = float32(m + y).  A cluster
 * falls back to means[k], bit for bit, when t or det is not finite or not > 0, or a |y_a| is not finite or > cell.  A cluster
 * with more than 2^15 (face, cluster) pairs is not placed (pos = mean) and sets the status 2.  vert_src_out [n_verts]: the member
 * with the smallest float32 squared distance to pos_out[k] (evaluated in double), ties to the lowest id.  qcounts (device
 * int32[4]) = clusters that fell back, pairs, the longest segment, status.  Rows of pos_out and vert_src_out from K on are ZERO.
 * Integer atomics only: the result is unique, and equal to meshing.mesh_quadric_place bit for bit.  cell finite and > 0, reg
 * finite and >= 0, n_verts <= 2^26, n_faces <= 2^28, otherwise ARAH_E_BADARG without a launch, and a scratch size of 0 for sizes
 * out of range; scratch: arah_mesh_quadric_place_scratch_bytes(n_verts, n_faces) device bytes, 256-byte aligned,
 * ARAH_E_WORKSPACE when short.  Empty inputs still write qcounts; pointers of empty arrays may be NULL.  No host synchronisation,
 * no allocation. */
size_t arah_mesh_quadric_place_scratch_bytes(int64_t n_verts, int64_t n_faces);
int arah_mesh_quadric_place(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int32_t* vert_map,
                            const float* means, const int32_t* counts, float cell, double reg, float* pos_out,
                            int32_t* vert_src_out, int32_t* qcounts, void* scratch, size_t scratch_bytes, void* stream);
/* Adjacency of an indexed mesh (csrc/meshadj.hpp).  faces [n_faces][3] vertex ids.  A face is VALID when its three ids lie in
 * [0, n_verts) and are pairwise different; the others are skipped.  A valid face (a, b, c) traverses the directed edges a->b,
 * b->c, c->a.  -> vf_start [n_verts + 1], vf [3 n_faces]: the CSR of the valid faces incident to every vertex, face ids ASCENDING
 * within a vertex; nbr_start [n_verts + 1], nbr [6 n_faces]: the CSR of the UNIQUE neighbours of every vertex, ids ascending;
 * nbr_out, nbr_in [6 n_faces]: for the entry (v, n) the number of valid faces traversing v->n and n->v; vert_flags [n_verts]
 * uint8: bit 0 the vertex has an edge with exactly one face, bit 1 an edge with three or more, bit 2 no neighbour; counts (device
 * int32[8]) = valid faces, undirected edges E, edges with one face (boundary), with >= 3 faces (non-manifold), with exactly two
 * faces that traverse it in the same direction (misoriented), the largest number of neighbours of a vertex, vertices with no
 * neighbour, the Euler characteristic (n_verts - counts[6]) - E + counts[0].  Rows of vf from vf_start[n_verts] on and of nbr,
 * nbr_out, nbr_in from nbr_start[n_verts] on are ZERO.  Integer atomics only, and they decide nothing but a layout that is
 * sorted afterwards: the result is unique.  Segments of any length are sorted (a workgroup per long one).  0 <= n_verts <=
 * INT32_MAX, 0 <= n_faces <= 2^28 (6 n_faces fits an int32), otherwise ARAH_E_BADARG without a launch and a scratch size of 0;
 * scratch: arah_mesh_adjacency_scratch_bytes(n_verts, n_faces) device bytes, 256-byte aligned, ARAH_E_WORKSPACE when short.
 * Empty inputs still write vf_start, nbr_start and counts; pointers of empty arrays may be NULL.  No host synchronisation, no
 * allocation. */
size_t arah_mesh_adjacency_scratch_bytes(int64_t n_verts, int64_t n_faces);
int arah_mesh_adjacency(const int32_t* faces, int64_t n_faces, int64_t n_verts, int32_t* vf_start, int32_t* vf, int32_t* nbr_start,
                        int32_t* nbr, int32_t* nbr_out, int32_t* nbr_in, uint8_t* vert_flags, int32_t* counts, void* scratch,
                        size_t scratch_bytes, void* stream);
/* One round of edge-collapse decimation of an indexed mesh (csrc/meshcollapse.hpp).  verts [n_verts][3], faces [n_faces][3]
 * vertex ids; the adjacency of the mesh is built inside the call (arah_mesh_adjacency's launches, in this call's scratch).  A
 * vertex is PINNED when a coordinate is not finite, when it has no neighbour, or when one of its neighbour entries is not "one
 * face each way".  The neighbour entry i = (u, v) with v > u names the edge {u, v}, i is its id.  An edge is a candidate unless,
 * in this order: (1) an end is pinned; (2) the third vertices a, b of its two faces are equal, or the two neighbour lists have
 * other than two ids in common, or a or b has fewer than four neighbours; (3) the faces that touch u or v, each once, number
 * more than 32; (4) with m the midpoint in double, the ten numbers of those faces about m (arah_mesh_quadric_place's nine and c
 * = d d) summed by its tree in ascending face id, y its solve with reg and the bound max_a |u_a - v_a| (y = 0 after a fall-back,
 * which is counted), pos = float32(m + y), raw = (y.Ay + 2 b.y) + c with every row and dot product summed left to right: the
 * float32 of raw is not finite; (5) cost32 = float32(raw), +0 unless raw > 0, exceeds max_cost; (6) a face that names one of u, v
 * has (N0 N'0 + N1 N'1) + N2 N'2 <= 0 (or not a number), N and N' its cross products before and after that corner moves to
 * pos.  key = (bits(cost32) << 32) | i; m1[x] = the least key of the candidates at x, m2[x] = the least of m1 over x and its
 * neighbours; a candidate is selected when m2[u] = m2[v] = key, and the first `need` selected edges in ascending id are applied:
 * v becomes u, u moves to pos, vert_src of u is the one of u, v with the smaller float32 squared distance to pos (u on a tie),
 * the valid faces that name both ends go, every other face keeps its row order and orientation with its ids in [0, n_verts)
 * renamed, the merged vertices go and the others keep their order.  -> verts_out [n_verts][3], vert_src [n_verts], faces_out
 * [n_faces][3], face_src [n_faces] (rows past the counts ZERO); counts (device int32[12]) = vertices, faces, selected edges,
 * applied edges, candidates, edges with reason 1 .. 6, fall-backs; edge_pos [6 n_faces][3], edge_key [6 n_faces] (all ones: no
 * candidate), edge_reason [6 n_faces] (0 candidate, 1 .. 6, 255: the entry names no edge) for every neighbour entry.  Integer
 * atomics only (min, add): the result is unique, and equal to meshing.mesh_collapse_round bit for bit.  need >= 0, reg finite
 * and >= 0, max_cost >= 0 (infinity: no bound), sizes as for arah_mesh_adjacency, otherwise ARAH_E_BADARG without a launch and a
 * scratch size of 0; scratch: arah_mesh_collapse_round_scratch_bytes(n_verts, n_faces) device bytes, 256-byte aligned,
 * ARAH_E_WORKSPACE when short.  Empty inputs still write counts; pointers of empty arrays may be NULL.  No host synchronisation,
 * no allocation. */
size_t arah_mesh_collapse_round_scratch_bytes(int64_t n_verts, int64_t n_faces);
int arah_mesh_collapse_round(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, int32_t need, double reg,
                             float max_cost, float* verts_out, int32_t* faces_out, int32_t* vert_src, int32_t* face_src,
                             int32_t* counts, float* edge_pos, uint64_t* edge_key, uint8_t* edge_reason, void* scratch,
                             size_t scratch_bytes, void* stream);
/* arah_mesh_collapse_round with two bounds on lengths, over the same kernels and the same scratch.  Before every other test: (7)
 * the edge's squared length (dx dx + dy dy) + dz dz in double is not below short_len2 (or not a number).  After test (6): (8) a
 * corner other than u and v of a face that names one of them lies farther than long_len2 (squared, in double, summed the same
 * way) from pos.  counts is device int32[14]: the twelve above, then the edges with reason 7 and with reason 8; edge_reason
 * takes 7 and 8 too.  Equal to meshing.mesh_collapse_round(short_len2=, long_len2=) bit for bit.  short_len2 >= 0 and long_len2
 * >= 0 (infinity: no bound), otherwise ARAH_E_BADARG; everything else as above. */
int arah_mesh_collapse_round_bounded(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, int32_t need, double reg,
                                     float max_cost, double short_len2, double long_len2, float* verts_out, int32_t* faces_out,
                                     int32_t* vert_src, int32_t* face_src, int32_t* counts, float* edge_pos, uint64_t* edge_key,
                                     uint8_t* edge_reason, void* scratch, size_t scratch_bytes, void* stream);
/* One round of subdivision of an indexed mesh (csrc/meshsubdiv.hpp).  verts [n_verts][3], faces [n_faces][3] vertex ids; the
 * adjacency of the mesh is built inside the call (arah_mesh_adjacency's launches, in this call's scratch).  The neighbour entry
 * (lo, hi) with hi > lo names an edge.  has_threshold = 0: every edge is marked; otherwise an edge is marked when both ends are
 * finite and (dx dx + dy dy) + dz dz > max_len2 in float64, every operation rounded on its own.  The k-th marked edge in entry
 * order becomes vertex n_verts + k; old vertices keep their ids.  method 0 (midpoint): old vertices are copied, a new one is
 * float32((lo + hi) 0.5), or the bits of its lowest non-finite end.  method 1 (Loop, Warren's weights; has_threshold must be 0):
 * a new vertex on an edge with one face each way and a finite stencil is float32((lo + hi) 0.375 + (c + d) 0.125), c and d the
 * third corners of the faces traversing lo->hi and hi->lo, every other one the midpoint; a finite old vertex whose k edges all
 * have one face each way and whose neighbours are finite moves to float32(p (1 - k beta) + s beta), s the sum of the neighbours in
 * ascending id, beta = 3/16 for k = 3 and 3 / (8 k) otherwise; a finite old vertex with exactly two one-face edges, finite
 * neighbours b0 < b1 across them and every other edge one face each way moves to float32(p 0.75 + (b0 + b1) 0.125); the others
 * stay.  A valid face with m marked edges becomes 1 + m faces in its orientation and the input's order (the templates of
 * meshing.mesh_subdivide_round; the quad of the two-mark template is cut along its shorter diagonal on the output positions,
 * ties to x-c); an invalid face is copied.  -> verts_out [n_verts + 3 n_faces][3], vert_src [n_verts + 3 n_faces][2] ((v, v) or
 * (lo, hi)), faces_out [4 n_faces][3], face_src [4 n_faces] (rows past the counts ZERO); counts (device int32[13]) = vertices
 * out, faces out, edges, marked edges, faces with 0 / 1 / 2 / 3 marks, invalid faces, marked edges with a non-finite end,
 * interior vertices moved, rim vertices moved, vertices kept.  No atomics besides the adjacency's: the result is unique, and
 * equal to meshing.mesh_subdivide_round bit for bit.  n_faces <= 2^26 and n_verts + 3 n_faces < 2^31, method 0 or 1, max_len2
 * >= 0 (infinity: nothing is marked), otherwise ARAH_E_BADARG without a launch and a scratch size of 0; scratch:
 * arah_mesh_subdivide_round_scratch_bytes(n_verts, n_faces) device bytes, 256-byte aligned, ARAH_E_WORKSPACE when short, without
 * a launch.  Empty inputs still write counts; pointers of empty arrays may be NULL.  No host synchronisation, no allocation. */
size_t arah_mesh_subdivide_round_scratch_bytes(int64_t n_verts, int64_t n_faces);
int arah_mesh_subdivide_round(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, int32_t method,
                              int32_t has_threshold, double max_len2, float* verts_out, int32_t* faces_out, int32_t* vert_src,
                              int32_t* face_src, int32_t* counts, void* scratch, size_t scratch_bytes, void* stream);
/* One round of edge flips of an indexed mesh (csrc/meshflip.hpp).  verts [n_verts][3], faces [n_faces][3] vertex ids; the
 * adjacency of the mesh is built inside the call (arah_mesh_adjacency's launches, in this call's scratch).  The neighbour entry
 * i = (u, v) with v > u names the edge {u, v}, i is its id.  An edge is a candidate unless, in this order: (1) the entry does not
 * carry one face each way; (2) a = b, the third corners of the faces traversing u->v (fa) and v->u (fb); (3) b is a neighbour of
 * a; (4) one of u, v, a, b has a non-finite coordinate; (5) the criterion does not ask for the flip -- criterion 0 (Delaunay):
 * with Na = (u - a) x (v - a), Nb = (v - b) x (u - b), d_x = (u - x).(v - x) and c_x = |N_x|^2 in double, every operation rounded
 * on its own and sums taken left to right, it asks when d_a < 0 and d_b < 0, never when both are >= 0, and otherwise when
 * (d_n d_n) c_o > (d_o d_o) c_n, n the corner with the negative d and o the other -- and the same test of the flipped edge {a,
 * b} with the corners u, v and the new faces' cross products must NOT ask (rounding lets a nearly co-circular quad ask both
 * ways); criterion 1 (valence): with deg the number
 * of neighbours and the target 4 for a vertex on a boundary (vert_flags bit 0) and 6 otherwise, it asks when the sum of |deg -
 * target| over u, v, a, b is strictly smaller with u, v one lower and a, b one higher; (6) one of the cross products of the
 * corners (a, u, b) and (b, v, a) has a dot product <= 0 (or not a number) with Na or Nb.  key = (hash32(i ^ salt 0x9e3779b9) <<
 * 32) | i with hash32(x): x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16 on 32-bit integers.  lock[x] =
 * the least key of the candidates with x among u, v, a, b; a candidate is selected when its four locks hold its key, so selected
 * flips share no vertex.  -> faces_out [n_faces][3]: the input's rows, row fa = (a, u, b) and row fb = (b, v, a) for a selected
 * edge; face_flag [n_faces]: 1 for a rewritten row; counts (device int32[9]) = edges, candidates, selected, edges with reason 1
 * .. 6; edge_key [6 n_faces] (all ones: no candidate), edge_reason [6 n_faces] (0 candidate, 1 .. 6, 255: the entry names no
 * edge) for every neighbour entry.  Integer atomics only (min, add): the result is unique, and equal to meshing.mesh_flip_round
 * bit for bit.  criterion 0 or 1, sizes as for arah_mesh_adjacency, otherwise ARAH_E_BADARG without a launch and a scratch size
 * of 0; scratch: arah_mesh_flip_round_scratch_bytes(n_verts, n_faces) device bytes, 256-byte aligned, ARAH_E_WORKSPACE when
 * short, without a launch.  Empty inputs still write counts; pointers of empty arrays may be NULL.  No host synchronisation, no
 * allocation. */
size_t arah_mesh_flip_round_scratch_bytes(int64_t n_verts, int64_t n_faces);
int arah_mesh_flip_round(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, int32_t criterion, uint32_t salt,
                         int32_t* faces_out, uint8_t* face_flag, int32_t* counts, uint64_t* edge_key, uint8_t* edge_reason,
                         void* scratch, size_t scratch_bytes, void* stream);
/* Per-vertex normals of an indexed mesh from the mesh itself (pytorch3d verts_normals_packed): verts [n_verts][3], faces
 * [n_faces][3], vf_start / vf of arah_mesh_adjacency on the same mesh.  Vertex v walks its incident faces in the order of vf
 * (ascending id); a face with a non-finite corner contributes nothing, the others (p1 - p0) x (p2 - p0) with the corners widened to
 * double, every operation rounded on its own; the sum starts at 0 and is taken in that order.  -> normal_sum [n_verts][3] double:
 * the sums; normals [n_verts][3] float: float(sum / sqrt((x x + y y) + z z)), (0, 0, 0) when that length is 0 or not finite.  A
 * gather: no atomics, no scratch.  A row of vf that names no valid face is skipped.  Sizes and errors as for arah_mesh_adjacency;
 * n_verts = 0 launches nothing. */
int arah_mesh_vertex_normals(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int32_t* vf_start,
                             const int32_t* vf, double* normal_sum, float* normals, void* stream);
/* Umbrella smoothing: n_steps steps over verts [n_verts][3] with nbr_start / nbr / vert_flags of arah_mesh_adjacency, all inside
 * this call.  Step i has the factor f = double(h_factors[i & 1]) (Taubin: {lambda, mu}; plain Laplacian: {lambda, lambda}).  A
 * vertex moves when it is finite, is not pinned (pin != 0 pins the vertices with vert_flags bit 0 or 1) and has a finite
 * neighbour: s = the double sum of its finite neighbours in the order of nbr (ascending id), m their number, new = float(p + f (s /
 * m - p)) in double, every operation rounded on its own; every other vertex is copied bit for bit.  A step reads the previous
 * step's positions only: the steps alternate between tmp [n_verts][3] and verts_out so that the LAST one writes verts_out; verts
 * is never written, tmp may be NULL for n_steps <= 1, and n_steps = 0 copies verts to verts_out.  A gather: no atomics.
 * ARAH_E_BADARG for n_verts outside [0, INT32_MAX], n_steps < 0, a factor that is not finite or a missing pointer; n_verts = 0
 * launches nothing. */
int arah_mesh_smooth(const float* verts, int64_t n_verts, const int32_t* nbr_start, const int32_t* nbr, const uint8_t* vert_flags,
                     int32_t n_steps, const float h_factors[2], int32_t pin, float* tmp, float* verts_out, void* stream);
/* One step of tangential relaxation of an indexed mesh: arah_mesh_smooth's gather with the part of the move along the vertex
 * normal taken out.  nbr_start / nbr / vert_flags of arah_mesh_adjacency and normal_sum [n_verts][3] (double) of
 * arah_mesh_vertex_normals on the same mesh.  A vertex moves when it is finite, has neither bit 0 nor bit 1 of vert_flags, has a
 * finite neighbour, and nn = (N0 N0 + N1 N1) + N2 N2 of its normal_sum N is finite and > 0: s = the double sum of its finite
 * neighbours in ascending id, m their number, d = s / m - p, t = ((d0 N0 + d1 N1) + d2 N2) / nn, new = float32(p + factor (d -
 * t N)) in double, every operation rounded on its own; no square root.  All other vertices are copied bit for bit.  -> verts_out
 * [n_verts][3], equal to meshing.mesh_tangential_step bit for bit.  A gather: no atomics, no scratch.  factor finite, n_verts <
 * 2^31, otherwise ARAH_E_BADARG without a launch.  No host synchronisation, no allocation. */
int arah_mesh_tangential(const float* verts, int64_t n_verts, const int32_t* nbr_start, const int32_t* nbr, const uint8_t* vert_flags,
                         const double* normal_sum, float factor, float* verts_out, void* stream);
/* The cotangent Laplacian of an indexed mesh (csrc/meshlaplace.hpp; meshing.mesh_cotangent is the rule, bit for bit except
 * angle_sum, whose atan2 is the only function that is not correctly rounded).  verts [n_verts][3], faces [n_faces][3], vf_start /
 * vf / nbr_start / nbr of arah_mesh_adjacency on the same mesh, mass 0 (barycentric) or 1 (mixed Voronoi).  -> weight [6 n_faces]
 * double, aligned with nbr: half the sum of the cotangents opposite to the edge over its faces in ascending face id, rows from
 * nbr_start[n_verts] on +0; diag, area, angle_sum [n_verts] double: the row sums in ascending neighbour id, the lumped mass, the sum
 * of the angles at the vertex in ascending face id; counts [8]: contributing, degenerate and nonfinite faces, contributing faces
 * with an obtuse corner, entries n > v with weight < 0, vertices whose area is not > 0, 0, 0.  A gather: a vertex's own lane or
 * workgroup writes its rows, integer atomics for the counts only, no scratch.  Rows of the caller's CSRs are clamped to the
 * arrays and ids tested before they are followed.  Sizes as for arah_mesh_adjacency; a mass other than 0 or 1 or a missing
 * pointer: ARAH_E_BADARG without a launch.  n_verts = 0 or n_faces = 0 still write counts (and zero rows). */
int arah_mesh_cotangent(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int32_t* vf_start,
                        const int32_t* vf, const int32_t* nbr_start, const int32_t* nbr, int32_t mass, double* weight, double* diag,
                        double* area, double* angle_sum, int32_t* counts, void* stream);
/* y = L x over the weights of arah_mesh_cotangent: x [n_verts][n_channels] float (x_is_f64 = 0) or double (1), 1 <= n_channels <=
 * 32; y [n_verts][n_channels] double, y[v][c] = the sum over v's entries in ascending neighbour id, from 0, of weight (x[n][c] -
 * x[v][c]), every operation rounded on its own; an entry whose weight or x[n][c] is not finite is skipped; the quiet NaN
 * 0x7ff8000000000000 where x[v][c] is not finite.  n_faces gives the rows
 * of nbr and weight (6 n_faces).  A gather, one thread per element of y.  ARAH_E_BADARG without a launch otherwise. */
int arah_mesh_laplacian_apply(const double* weight, const int32_t* nbr_start, const int32_t* nbr, int64_t n_verts, int64_t n_faces,
                              const void* x, int32_t x_is_f64, int32_t n_channels, double* y, void* stream);
/* Curvatures from weight / area / angle_sum of arah_mesh_cotangent, normal_sum of arah_mesh_vertex_normals and vert_flags of
 * arah_mesh_adjacency (meshing.mesh_curvature is the rule, bit for bit given the same angle_sum).  L = arah_mesh_laplacian_apply of
 * the positions, K = (-L) / area; -> curv [n_verts][5] double: mean = 0.5 ((K.N) / |N|), mean_abs = 0.5 |K|, gaussian = ((2 pi, or
 * pi with vert_flags bit 0) - angle_sum) / area, k1, k2 = mean +- sqrt(max(mean mean - gaussian, 0)); mean_normal [n_verts][3]
 * double = 0.5 K; valid [n_verts]; counts [1]: the invalid vertices.  A vertex with vert_flags bit 1 or 2, a non-finite
 * coordinate, an area or |N| that is not finite and > 0 is invalid: NaN everywhere, valid = 0.  One thread per vertex. */
int arah_mesh_curvature(const float* verts, int64_t n_verts, int64_t n_faces, const int32_t* nbr_start, const int32_t* nbr,
                        const uint8_t* vert_flags, const double* weight, const double* area, const double* angle_sum,
                        const double* normal_sum, double* curv, double* mean_normal, uint8_t* valid, int32_t* counts, void* stream);
/* arah_mesh_smooth with cotangent weights: every step recomputes the weights from the positions it reads (into the scratch) and
 * uses the entries with a finite neighbour and a finite weight.  A vertex moves when it is finite, is not pinned and s = the sum
 * of |w| over those entries in ascending neighbour id is finite and > 0: new = float(p + f ((sum of w (q - p)) / s)) in double.
 * Factors, pin, tmp and verts_out as for arah_mesh_smooth.  scratch: arah_mesh_smooth_cotangent_scratch_bytes(n_verts, n_faces)
 * device bytes, ARAH_E_WORKSPACE when short; ARAH_E_BADARG as for arah_mesh_smooth, both without a launch. */
size_t arah_mesh_smooth_cotangent_scratch_bytes(int64_t n_verts, int64_t n_faces);
int arah_mesh_smooth_cotangent(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int32_t* vf_start,
                               const int32_t* vf, const int32_t* nbr_start, const int32_t* nbr, const uint8_t* vert_flags, int32_t n_steps,
                               const float h_factors[2], int32_t pin, float* tmp, float* verts_out, void* scratch, size_t scratch_bytes,
                               void* stream);
/* Systems with the cotangent operator, by Jacobi-preconditioned conjugate gradients in double (csrc/meshsolve.hpp;
 * meshing.laplacian_solve is the rule, bit for bit).  weight / area of arah_mesh_cotangent, nbr_start / nbr of arah_mesh_adjacency;
 * rhs, x0, x [n_verts][n_channels] double, 1 <= n_channels <= 32; pinned [n_verts] bytes or null; mass_coef >= 0, stiff_coef > 0,
 * tol >= 0, all finite.  At every SOLVED vertex mass_coef area x - stiff_coef sum w (x_n - x) = rhs over the usable entries (finite
 * weight, x0 row of the neighbour finite), x = x0 at every other; classes [n_verts]: 0 solved, 1 pinned, 2 x0 row not finite, 3 rhs
 * row not finite, 4 area not finite and > 0 (mass_coef != 0 only), 5 diagonal not finite and > 0; counts [8]: the vertices by
 * class, 0, 0.  Per column: iters, status (0 running, 1 converged: rr <= tol^2 r0, 2 breakdown: r0 or p.Ap not finite and > 0), rr
 * = the squared residual, r0 = its first value.  Inner products are the fixed tree of arah_mesh_quadric_place over the vertices
 * as one segment: workgroup trees over blocks of 256, then one workgroup per column; no floating-point atomics.
 * arah_mesh_solve_begin writes x = x0, the classes and the start state into the scratch, and the outputs (a null output is
 * skipped); arah_mesh_solve_steps takes n_steps steps of four launches each on that scratch with the same operator arguments, a
 * stopped column is left alone, and iters / status / rr / r0 are written again.  No host synchronisation, no allocation.
 * scratch: arah_mesh_solve_scratch_bytes(n_verts, n_channels) device bytes (0 for sizes that are refused), ARAH_E_WORKSPACE
 * when short.  n_verts <= 2^24 (a longer tree needs a level more), sizes otherwise as for arah_mesh_adjacency; a bad size,
 * coefficient or a missing pointer: ARAH_E_BADARG.  Refused calls launch nothing. */
size_t arah_mesh_solve_scratch_bytes(int64_t n_verts, int64_t n_channels);
int arah_mesh_solve_begin(const double* weight, const double* area, const int32_t* nbr_start, const int32_t* nbr, int64_t n_verts,
                          int64_t n_faces, const double* rhs, const double* x0, const uint8_t* pinned, int32_t n_channels, double mass_coef,
                          double stiff_coef, double tol, double* x, int32_t* iters, int32_t* status, double* rr, double* r0,
                          int32_t* counts, uint8_t* classes, void* scratch, size_t scratch_bytes, void* stream);
int arah_mesh_solve_steps(const double* weight, const double* area, const int32_t* nbr_start, const int32_t* nbr, int64_t n_verts,
                          int64_t n_faces, int32_t n_channels, double mass_coef, double stiff_coef, int32_t n_steps, double* x,
                          int32_t* iters, int32_t* status, double* rr, double* r0, void* scratch, size_t scratch_bytes, void* stream);
/* Consistent orientation of an indexed mesh (csrc/meshorient.hpp; meshing.mesh_orient is the rule, bit for bit).  faces
 * [n_faces][3], and vf_start / vf / nbr_start / nbr / nbr_out / nbr_in of arah_mesh_adjacency on the same mesh.  Two valid faces are
 * neighbours across an edge that carries exactly two valid faces, consistent when they traverse it in opposite directions; the
 * orientation components are the classes of faces connected through such edges, numbered in ascending order of their lowest
 * face; the double cover (nodes 2 f + bit) gives b(f), the flip of f relative to that lowest face, and marks the non-orientable
 * components, whose faces are never flipped.  policy: 0 seed (the lowest face keeps its orientation), 1 majority (the orientation
 * held by more faces wins, ties to seed), 2 negative / 3 positive (the component's integer volume gets that sign; a zero volume
 * falls back to majority).  The volume: q = llrint(clamp((double(v) - double(h_origin)) scale, -2^18, 2^18)), the sum of
 * det(q0, q1, q2) in int64 over the faces as the seed orients them, a face with a non-finite vertex contributing nothing; verts
 * [n_verts][3], h_origin and scale are read under the policies 2 and 3 only (and may be NULL / anything otherwise).  -> flip
 * [n_faces] uint8; face_comp [n_faces] (-1: an invalid face); faces_out [n_faces][3]: a flipped row (a, b, c) is (a, c, b), every
 * other row is copied; comp_faces, comp_flags (bit 0 non-orientable, bit 1 reversed by the policy) [n_faces] int32 and comp_vol_hi,
 * comp_vol_lo [n_faces] int64 (the volume is hi 2^32 + lo; zero under the policies 0 and 1), indexed by component, ZERO from the
 * number of components on; counts (device int32[6]) = valid faces, components, non-orientable components, faces with b = 1,
 * components reversed, faces flipped.  Integer atomics only (min, add): the result is unique.  Sizes and errors as for
 * arah_mesh_adjacency; scratch: arah_mesh_orient_scratch_bytes(n_verts, n_faces) device bytes.  n_faces = 0 still writes counts.
 * No host synchronisation, no allocation. */
size_t arah_mesh_orient_scratch_bytes(int64_t n_verts, int64_t n_faces);
int arah_mesh_orient(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int32_t* vf_start, const int32_t* vf,
                     const int32_t* nbr_start, const int32_t* nbr, const int32_t* nbr_out, const int32_t* nbr_in, int32_t policy,
                     const float h_origin[3], double scale, uint8_t* flip, int32_t* face_comp, int32_t* faces_out, int32_t* comp_faces,
                     int32_t* comp_flags, int64_t* comp_vol_hi, int64_t* comp_vol_lo, int32_t* counts, void* scratch,
                     size_t scratch_bytes, void* stream);
/* Boundary loops of an indexed mesh (meshing.mesh_boundary_loops is the rule).  A boundary half-edge is a directed edge a->b of a
 * valid face whose undirected edge carries exactly one valid face (nbr_start / nbr / nbr_out / nbr_in of arah_mesh_adjacency); they
 * are numbered in ascending (face, corner) order.  A loop is a connected component of them through shared vertex ids; loops are
 * numbered in ascending order of their smallest vertex; a loop is simple when every vertex on it has exactly one outgoing and one
 * incoming boundary half-edge.  -> edges [3 n_faces][2], edge_face, edge_loop [3 n_faces]; loop_edges, loop_vert (the smallest
 * vertex) [n_verts] int32 and loop_simple [n_verts] uint8, indexed by loop; counts (device int32[3]) = boundary half-edges B,
 * loops L, simple loops.  Rows from B and from L on are ZERO.  Integer atomics only.  Sizes and errors as for arah_mesh_adjacency;
 * scratch: arah_mesh_boundary_loops_scratch_bytes(n_verts, n_faces).  Empty inputs still write counts. */
size_t arah_mesh_boundary_loops_scratch_bytes(int64_t n_verts, int64_t n_faces);
int arah_mesh_boundary_loops(const int32_t* faces, int64_t n_faces, int64_t n_verts, const int32_t* nbr_start, const int32_t* nbr,
                             const int32_t* nbr_out, const int32_t* nbr_in, int32_t* edges, int32_t* edge_face, int32_t* edge_loop,
                             int32_t* loop_edges, uint8_t* loop_simple, int32_t* loop_vert, int32_t* counts, void* scratch,
                             size_t scratch_bytes, void* stream);
/* Small holes closed by a fan (meshing.mesh_fill_holes is the rule): edges, edge_loop, loop_edges, loop_simple, loop_vert and
 * loop_counts are the arrays of arah_mesh_boundary_loops on the same mesh.  A loop is filled when it is simple, 3 <= loop_edges <=
 * max_edges (0 <= max_edges <= 2^26) and none of its vertices has a non-finite coordinate.  Filled loop number j (in loop order)
 * adds the vertex n_verts + j at the fixed-point mean of the loop's vertices -- the rule of arah_mesh_simplify: q =
 * llrint(clamp((double(v) - double(h_origin)) fix_scale, -2^36, 2^36)), float(double(h_origin) + (double(sum q) / double(n)) /
 * fix_scale) -- and every half-edge a->b of a filled loop adds, in edge order, the face (b, a, new vertex) behind the n_faces old
 * ones.  -> verts_out [n_verts + n_verts / 3][3], vert_src [n_verts + n_verts / 3] (an old vertex: itself; a new one: its loop's
 * smallest vertex), faces_out [4 n_faces][3], face_loop [4 n_faces] (-1 for the old faces); counts (device int32[5]) = B, L, simple
 * loops, filled loops, faces added.  Rows behind the filled loops and the added faces are ZERO.  Integer atomics only.  Sizes
 * and errors as for arah_mesh_adjacency; scratch: arah_mesh_fill_holes_scratch_bytes(n_verts, n_faces). */
size_t arah_mesh_fill_holes_scratch_bytes(int64_t n_verts, int64_t n_faces);
int arah_mesh_fill_holes(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int32_t* edges,
                         const int32_t* edge_loop, const int32_t* loop_edges, const uint8_t* loop_simple, const int32_t* loop_vert,
                         const int32_t* loop_counts, int32_t max_edges, const float h_origin[3], double fix_scale, float* verts_out,
                         int32_t* vert_src, int32_t* faces_out, int32_t* face_loop, int32_t* counts, void* scratch, size_t scratch_bytes,
                         void* stream);
/* An indexed mesh drawn (csrc/meshraster.hpp; meshing.mesh_rasterize is the rule, bit for bit): verts [n_verts][3] = (u, v, view
 * depth) in pixel coordinates (pixel (i, j) has its centre at u = j + 0.5, v = i + 0.5), faces [n_faces][3].  A face is valid when
 * its ids lie in [0, n_verts), its z are finite and > z_near and area2 = (x1-x0)(y2-y0) - (x2-x0)(y1-y0) is finite and not 0; cull
 * = 0 none, 1 drops area2 < 0, 2 drops area2 > 0.  With e0 = E(1,2), e1 = E(2,0), e2 = E(0,1), E(a,b) = (xa-px)(yb-py) -
 * (xb-px)(ya-py), every float operation rounded on its own, a pixel centre inside the closed bounding box is covered when all e_k
 * >= 0 (area2 > 0) or all <= 0 (area2 < 0) and s = (e0+e1)+e2 != 0: faces that share an edge leave no centre uncovered.  The
 * fragment's depth is z = 1 / (((e0/z0 + e1/z1) + e2/z2) / s); the smallest key (bits(z) << 32) | face wins the pixel.  ->
 * pix_to_face [H][W] (-1: nothing), depth [H][W] (the key's z; -1), bary [H][W][3] (perspective-correct, from the same e_k in
 * double; -1).  keys [H*W] is scratch, initialised inside the call.  Two passes: a scatter with a 64-bit integer atomicMin (the
 * only atomic that decides anything: the result does not depend on the order of arrival) and a per-pixel resolve.  A face's
 * clipped bounding box is drawn whatever its size: by its lane, by its wave, by a workgroup or by 64 of them.  pix_to_face, depth
 * and bary[0..1] hold the lists of the larger faces between the passes.  ARAH_E_BADARG for a negative count or one above INT32_MAX, H or W <= 0,
 * H W above INT32_MAX, an unknown cull code or a missing pointer; n_faces = 0 or n_verts = 0 writes the background. */
int arah_mesh_rasterize(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, int32_t H, int32_t W, float z_near,
                        int32_t cull, uint64_t* keys, int32_t* pix_to_face, float* depth, float* bary, void* stream);
/* The same with the three thresholds of pass A given instead of built in: a face whose clipped bounding box has at most small_area
 * pixels is drawn by its lane, at most wave_area by its wave, at most huge_area by one workgroup, a larger one by 64 workgroups.
 * Every choice gives the same image; tools/mesh_render_bench.py measures them.  0 <= small_area <= wave_area <= huge_area. */
int arah_mesh_rasterize_debug(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, int32_t H, int32_t W,
                              float z_near, int32_t cull, int32_t small_area, int32_t wave_area, int32_t huge_area, uint64_t* keys,
                              int32_t* pix_to_face, float* depth, float* bary, void* stream);
/* Per-vertex attributes attr [n_verts][n_channels] drawn with the pix_to_face / bary of arah_mesh_rasterize: out [H][W][n_channels]
 * = float((b0 a0 + b1 a1) + b2 a2) in double, every operation rounded on its own; `background` where pix_to_face names no face of
 * this mesh or the face an id out of range.  1 <= n_channels <= 32.  Sizes and errors as for arah_mesh_rasterize. */
int arah_mesh_interpolate(const int32_t* pix_to_face, const float* bary, int32_t H, int32_t W, const int32_t* faces, int64_t n_faces,
                          const float* attr, int64_t n_verts, int32_t n_channels, float background, float* out, void* stream);
/* raw canonical x_hat [P,3] -> d x_bar / d x_hat [P,3,3] */
int arah_skin_jacobian(const ArahFrame* h_frame, const float* x_hat, int32_t n_pts, float* jac,
                       void* workspace, size_t workspace_bytes, void* stream);
/* x_norm [P,3], normal [P,3], view [P,3] (ignored for NO_VIEW_DIR), feat [P,256] -> rgb [P,3] */
int arah_color_eval(const ArahFrame* h_frame, const float* x_norm, const float* normal, const float* view,
                    const float* feat, int32_t n_pts, float* rgb, void* workspace, size_t workspace_bytes,
                    void* stream);
/* posed points [P,3] -> nearest vertex idx [P] (optional), raw canonical x_hat0 [P,3], T0 [P,16] */
int arah_nearest_inverse_lbs(const ArahFrame* h_frame, const float* pts, int32_t n_pts, int32_t* idx,
                             float* x_hat0, float* T0, void* workspace, size_t workspace_bytes, void* stream);
/* Broyden on g(x) = LBS(x) - tgt from caller-supplied x0 [P,3], T0 [P,16];
 * J^-1_0 = (sum_j w_j(x0) A_j)[:3,:3]^-1.  -> x [P,3] raw canonical, T [P,16], err [P] (optional), conv [P].
 * A point whose start is never improved keeps T0 -- rows 0..2 and T0[3][3] bit for bit; T0[3][0..2] must be zero (the
 * bottom row of an affine transform): the solver carries the target there and returns zeros.  n_pts = 0 is a no-op. */
int arah_broyden3_lbs(const ArahFrame* h_frame, const float* tgt, const float* x0, const float* T0,
                      int32_t n_pts, float* x, float* T, float* err, uint8_t* conv, int32_t canon_kernel /* ARAH_CANON_KERNEL_* */,
                      void* workspace, size_t workspace_bytes, void* stream);

/* joint root find on u = (x_hat, depth) from caller-supplied starts (search_iso_surface_depth, root_finding_utils.py:
 * 365-484): valid [N], x0 [N,3] raw canonical, z0 [N], T0 [N,16]  ->  x [N,3], z [N], T [N,16], conv [N].
 * Rays outside `valid` keep (x0, z0, T0) and are reported as not converged. */
int arah_joint_root_find(const ArahFrame* h_frame, const float* cam_loc, int32_t rays_per_cam, const float* dirs,
                         const uint8_t* valid, const float* x0, const float* z0, const float* T0, int32_t n_rays,
                         float* x, float* z, float* T, uint8_t* conv, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- loop D with gradients (training; get_rbg_value_vol_sdf with self.training, IDR:261-396) ---------
 * Per-sample forward (SDF value, normal, colour) and its hand-written backward incl. the second-order path through
 * the normal.  Compositing and the loss stay with the caller (autograd); this pair is the custom op in between. */
typedef struct ArahTrainIn {
    int32_t n;                  /* P valid samples, dense */
    int32_t rotate_normal;      /* !cano_view_dirs: the colour net sees R n with R = T[:3,:3] (IDR:339-340) */
    int32_t ray_augm;           /* IDR:342-350: where n . view <= 0 the un-augmented view is used */
    int32_t geom_only;          /* 1: SDF value and normal only (the regulariser queries of IDR:104-128): the forward returns the
                                   normal in rgb4[:, :3]; the backward takes dL/dn in g_rgb and writes the feature stream h_6
                                   to ArahTrainGrads.c[0]; T / view are ignored, no hand-over */
    const float* x;             /* [P,3] normalised canonical points */
    const float* T;             /* [P,16] forward transforms (rotate_normal) or NULL */
    const float* view;          /* [P,3] view input of the colour net */
    const float* view_orig;     /* [P,3] (ray_augm) or NULL */
    const float* g_s;           /* [P]   dL/d sdf (normalised units)   -- backward only */
    const float* g_rgb;         /* [P,3] dL/d rgb                      -- backward only */
    /* Optional hand-over from the forward to the backward call (all NULL: the backward recomputes the whole forward).
     * Forward: tap_cin / tap_c non-NULL -> the colour MLP's input and hidden activations are written there.  Backward:
     * the same buffers (they are also ArahTrainGrads.cin / .c) plus the forward's rgb -> the normal sweep and the colour
     * MLP are not recomputed (9 of the backward kernel's 34 layer products, all on the fp32 MFMA). */
    float* tap_cin;             /* [P,kInPad] */
    float* tap_c[5];            /* [P,256] [P,256] [P,128] [P,256] [P,256] */
    const float* fwd_rgb4;      /* [P,4] rgb of the forward call       -- backward only */
} ArahTrainIn;

/* Outputs of the backward.  Weight gradients are sums of outer products over all samples; the kernel streams their
 * operands as dense row-major [P,width] matrices and the caller finishes them with library GEMMs:
 *   dW_k = av[k]^T h[k] + avd[k]^T hd[k]  (k = 0..5, SDF layer k+1),  db_k = colsum(av[k]),
 *   dw_7 = g_s^T cin[:, :256] + colsum(hd[6]),  db_7 = sum(g_s),
 *   colour layer l: dW_l = d[l]^T X_l with X_0 = cin, X_1..X_2 = c[0..1], X_3 = [cin | c[2]], X_4..X_5 = c[3..4]. */
typedef struct ArahTrainGrads {
    float* sdf;                 /* [P]   forward values again (recomputed) */
    float* rgb4;                /* [P,4] */
    float* gx4;                 /* [P,4] dL/dx */
    float* film_freq;           /* [6,256] dL/d freq  */
    float* film_phase;          /* [6,256] dL/d phase */
    float* h[6];                /* h_0 [P,4] (x), h_1..h_5 [P,256] */
    float* hd[7];               /* tangent stream: hd_0 = dL/dn [P,4], hd_1..hd_6 [P,256] */
    float* av[6];               /* adj v_1..v_6 [P,256] */
    float* avd[6];              /* adj vd_1..vd_6 [P,256] */
    float* cin;                 /* [P,KIN_PAD] colour input, columns [feat(256) | x | n | PE(view) | 0] */
    float* c[5];                /* colour hidden activations: 256, 256, 128, 256, 256 wide */
    float* d[6];                /* colour deltas: 256, 256, 128, 256, 256 wide, delta_5 [P,4] */
} ArahTrainGrads;

size_t arah_shade_train_slab_bytes(void);   /* scratch of the backward (pre-activation spill, per workgroup) */
/* -> sdf [P] (normalised units), rgb4 [P,4] */
int arah_shade_train_forward(const ArahFrame* h_frame, const ArahTrainIn* h_in, float* sdf, float* rgb4,
                             void* workspace, size_t workspace_bytes, void* stream);
int arah_shade_train_backward(const ArahFrame* h_frame, const ArahTrainIn* h_in, const ArahTrainGrads* h_out,
                              void* slab, size_t slab_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* VolSDF density + alpha compositing of the TRAINING forward and their backward (IDR:363-394 with self.training): one
 * thread per ray over its `len[r]` valid samples, which are contiguous from `off[r]` in the compacted per-sample arrays
 * sdf [P] (metres), rgb [P,3], z [P].  inv_beta: device scalar 1 / beta.  acc is clip(sum of weights, 0, 1).  The
 * backward takes dL/d rgb_map [n_rays,3] and dL/d acc [n_rays] and returns dL/d sdf [P], dL/d rgb [P,3] and the scalar
 * dL/d inv_beta.  Replaces ~40 element-wise launches forward and ~100 backward of the autograd formulation. */
int arah_composite_train_forward(int32_t n_rays, int32_t n_steps, int32_t render_last_pt, const int32_t* len,
                                 const int64_t* off, const float* sdf, const float* rgb, const float* z, const float* inv_beta,
                                 float* out_rgb, float* out_acc, void* stream);
int arah_composite_train_backward(int32_t n_rays, int32_t n_steps, int32_t render_last_pt, const int32_t* len,
                                  const int64_t* off, const float* sdf, const float* rgb, const float* z, const float* inv_beta,
                                  const float* g_rgb_map, const float* g_acc, float* g_sdf, float* g_rgb, float* g_inv_beta,
                                  void* stream);

/* Skinny weight-gradient product of the training step: partial[blk][i][j] = sum over the block's rows p of
 * a[p*lda + i] * b[p*ldb + j], i < m <= 4, j < n; blk < arah_gram_skinny_blocks(n_rows).  The caller sums over blk.
 * (The reference leaves these to autograd's matmul backward: IDR:336-361 through torch.autograd.) */
int32_t arah_gram_skinny_blocks(int32_t n_rows);

/* y[r] = W[r, :] . x + b0[r] + b1[r]: the batch-1 output layers of the SDF hypernetwork (hyperlayers.py:418-465, 256 ->
 * in*out + out per emitted layer; im2mesh/metaavatar/models/siren_modules.py:244-300 calls them once per frame), an HBM
 * stream of the weight matrix.  W [n_rows][n_cols] row-major, 16-byte aligned, n_cols a multiple of 4; b0 / b1 [n_rows]
 * or NULL (bias of the layer, hypo_params_init).  Inference only (no gradient). */
int arah_gemv_rows(const float* W, int32_t n_rows, int32_t n_cols, const float* x, const float* b0, const float* b1,
                   float* y, void* stream);
int arah_gram_skinny(const float* a, int32_t lda, int32_t m, const float* b, int32_t ldb, int32_t n, int32_t n_rows,
                     float* partial, void* stream);

/* y[c] = sum over rows r of scale[r] * a[r*lda + c] (scale NULL: 1), c < n_cols: the bias gradients of the training step's tall
 * layers (sums of per-sample deltas over ~1.2e5 samples) and, with scale = the upstream gradient g and a = a hypernetwork head's
 * weight matrix [in*out + out][256], the head's input gradient g W -- the reference leaves both to autograd (sum / mm backward
 * of hyperlayers.py:418-465 and of the skinning decoder).  partial: arah_colsum_blocks(n_rows) * n_cols floats of scratch; the
 * partial sums are added in block order (deterministic).  One pass over `a` at HBM speed, no host synchronisation. */
int32_t arah_colsum_blocks(int64_t n_rows);
int arah_colsum(const float* a, int64_t lda, int32_t n_cols, int64_t n_rows, const float* scale, float* partial, float* y,
                void* stream);

/* Hierarchical softmax of the skinning queries of a training step with its backward (utils/utils.py:138-181, called from
 * root_finding_utils.py:54-113 with the 25 logits x 20): weights [n][24] = hsoftmax(scale * logits [n][25]);
 * g_logits [n][25] = d L / d logits for upstream gradients g_weights [n][24] (the forward is recomputed).  The reference runs the
 * recursion on autograd. */
int arah_hsoftmax_train_forward(const float* logits, int32_t n, float scale, float* weights, void* stream);
int arah_hsoftmax_train_backward(const float* logits, int32_t n, float scale, const float* g_weights, float* g_logits, void* stream);

/* HierarchicalPoseEncoder of one frame (im2mesh/metaavatar/models/siren_modules.py:196-244) with its backward, one launch each
 * way: n_joints MLPs 19 -> 19 -> ReLU -> 6 on [own (13: rotation 9, joint 3, bone length 1) | the parent's feature (6); the
 * root: glob (6) = layer_0's output], walked down the kinematic tree.  own [J][13], W1 [J][19][19], b1 [J][19], W2 [J][6][19],
 * b2 [J][6] (the per-joint nn.Linear parameters stacked, (out, in) row-major), parents_host [J] on the HOST (-1: root; parents
 * precede children), n_joints <= 64 -> feats [J][6], hidden [J][19] (post-ReLU, kept for the backward).
 * Backward: g_feats [J][6] -> gradients of the stacked parameters and of glob.  The reference runs the joints on autograd. */
int arah_pose_tree_forward(const float* own, const float* glob, const float* W1, const float* b1, const float* W2,
                           const float* b2, const int32_t* parents_host, int32_t n_joints, float* feats, float* hidden,
                           void* stream);
int arah_pose_tree_backward(const float* own, const float* glob, const float* W1, const float* W2, const int32_t* parents_host,
                            int32_t n_joints, const float* feats, const float* hidden, const float* g_feats, float* gW1,
                            float* gb1, float* gW2, float* gb2, float* g_glob, void* stream);

/* inv[p] = (scale * m[p])^-1 for n row-major 3 x 3 matrices (cofactors): the Jacobians d x_bar / d x_hat of the implicit
 * re-attachment of the canonical points to the skinning network (implicit_differentiable_renderer.py:315-334, torch.inverse
 * there).  A singular matrix gives non-finite entries, as torch.inverse does on the device. */
int arah_inverse3x3(const float* m, int32_t n, float scale, float* inv, void* stream);

/* Mesh queries of the training data path (zju_mocap.py:461-543): for every query point the closest point of the triangle
 * mesh -- squared distance, face (lowest index on ties), the point, barycentric weights of the face's three vertices
 * (igl.point_mesh_squared_distance + igl.barycentric_coordinates_tri) -- and containment exactly as
 * im2mesh/utils/libmesh/inside_mesh.py:4-100 decides it (z-ray crossing parity in both directions, hash resolution 512,
 * double precision).  verts [V,3] f32, faces [F,3] i32, pts [P,3] f32 or f64 -> d2 [P] f64, face [P] i32,
 * closest [P,3] f64, bary [P,3] f64, inside [P] u8.  scratch: arah_mesh_query_scratch_bytes() device bytes. */
size_t arah_mesh_query_scratch_bytes(void);
int arah_mesh_query(const float* verts, int32_t n_verts, const int32_t* faces, int32_t n_faces, const void* pts,
                    int32_t pts_are_f64, int32_t n_pts, double* d2, int32_t* face, double* closest, double* bary,
                    uint8_t* inside, void* scratch, void* stream);

/* PSNR and SSIM of a rendered frame against its ground-truth image (im2mesh/utils/eval.py:6-18; csrc/metrics.hpp), without a host
 * round trip.  pred / gt (H,W,3) fp32 interleaved, box_mask (H,W) uint8, non-zero = the frame's rays.  All arithmetic is float64 on
 * the fp32 pixels; no atomics: the same inputs give the same bits.
 *   mse  = mean over the masked pixels' 3 channels of (pred - gt)^2;  psnr = -10 log10(mse), +inf for mse == 0
 *   rect = bounding rectangle of the non-zero mask bytes (x, y, w, h as cv2.boundingRect), found on the device
 *   ssim = skimage.metrics.structural_similarity 0.18.1 (multichannel, 7 x 7 uniform window, sample covariance, C1 = (0.01 R)^2,
 *          C2 = (0.03 R)^2, mean over the window centres >= 3 pixels from every edge, then over the channels) on the crop
 *          [y:y+h, x:x+w] of both images, R = data_range (skimage's default for float images: 2).  Only windows wholly inside the
 *          crop are read, nothing outside it.
 * out [4] DEVICE doubles: psnr, ssim, mse, number of masked pixels.  rect [5] DEVICE: x, y, w, h, status -- 0 ok, 1 empty mask
 * (psnr, ssim, mse NaN; rect 0), 2 crop narrower or lower than 7 (ssim NaN, psnr / mse valid).  scratch:
 * arah_image_metrics_bytes(height, width) bytes, 8-byte aligned (the rectangle's bounds and per-workgroup partial sums and rectangles, folded
 * in index order).  No host synchronisation. */
size_t arah_image_metrics_bytes(int32_t height, int32_t width);
int arah_image_metrics(const float* pred, const float* gt, const uint8_t* box_mask, int32_t height, int32_t width,
                       double data_range, double* out, int32_t* rect, void* scratch, size_t scratch_bytes, void* stream);

/* Exact point-to-mesh distance against large triangle soups, and the geometry scores built on it (csrc/meshdist.hpp; no
 * reference counterpart: the reference's tree computes no geometry score).  tris [F,3,3] f32 with finite vertices.
 *   arah_mesh_index_build  a uniform grid of triangle references over the soup's bounding box, with a Chebyshev distance
 *                          transform of its occupied cells, into the caller's `index` buffer (arah_mesh_index_bytes(F) bytes,
 *                          256-byte aligned).  The buffer's size is fixed by F alone: a triangle is referenced from at most
 *                          8 cells, one that overlaps more is kept on a list every query walks.  Nothing is truncated.
 *   arah_mesh_closest      pts [P,3] f32 (finite) -> d2 [P] f64, face [P] i32, closest [P,3] f64 or NULL, tested [P] i32 or
 *                          NULL (point-triangle tests the query made).  d2 / face / closest are bit-equal to arah_mesh_query's
 *                          on the same triangles: the same per-triangle arithmetic, the lexicographic minimum of
 *                          (d2, face index).  A non-finite point or vertex gives d2 NaN, face -1.  `tris` must be the buffer
 *                          the index was built from.
 *   arah_surface_metrics   samples of mesh A queried against B and of B against A -> out [9] DEVICE doubles: accuracy,
 *                          completeness, chamfer_l1, chamfer_l2, normal_consistency, hausdorff_ab, hausdorff_ba, n_a, n_b.
 *                          sample_face_x [n_x] i32: the face of X each sample was drawn from; d2_xy / face_xy [n_x]: its query
 *                          result against Y.  Normals are the faces' float64 cross products, normalised; the sums run in
 *                          index order (no atomics).  scratch: arah_surface_metrics_bytes(n_a, n_b) bytes, 8-byte aligned.
 *   arah_face_area_cumsum  cum [F] f64: running sum of the triangles' areas (half the norm of the float64 cross product) in a
 *                          fixed order, for area-weighted sampling that gives the same bits on every run.
 * No host synchronisation anywhere. */
size_t arah_mesh_index_bytes(int32_t n_faces);
int arah_face_area_cumsum(const float* tris, int32_t n_faces, double* cum, void* stream);
int arah_mesh_index_build(const float* tris, int32_t n_faces, void* index, size_t index_bytes, void* stream);
int arah_mesh_closest(const void* index, size_t index_bytes, const float* tris, int32_t n_faces, const float* pts,
                      int32_t n_pts, double* d2, int32_t* face, double* closest, int32_t* tested, void* stream);
size_t arah_surface_metrics_bytes(int32_t n_a, int32_t n_b);
int arah_surface_metrics(const float* tris_a, int32_t n_faces_a, const int32_t* sample_face_a, const double* d2_ab,
                         const int32_t* face_ab, int32_t n_a, const float* tris_b, int32_t n_faces_b,
                         const int32_t* sample_face_b, const double* d2_ba, const int32_t* face_ba, int32_t n_b, double* out,
                         void* scratch, size_t scratch_bytes, void* stream);

/* Which faces of an indexed mesh cut through each other (csrc/meshintersect.hpp; no reference counterpart;
 * meshing.mesh_intersections is the rule, bit for bit).  verts [n_verts][3], faces [n_faces][3].  q = llrint(clamp((double(v) -
 * double(h_origin)) scale, -2^18, 2^18)) per coordinate; a face with an id outside [0, n_verts) or a non-finite vertex is VOID and
 * intersects nothing.  orient(a,b,c,d) = det[b-a; c-a; d-a] in int64 (below 2^60).  A segment pq properly crosses a triangle abc
 * when orient(a,b,c,p) and orient(a,b,c,q) are non-zero and of opposite sign and orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a)
 * are all >= 0 or all <= 0; two faces f != g intersect when an edge of one properly crosses the other, either way round.  Faces
 * that share a vertex or an edge are reported only when they fold through each other; duplicates, touching contact and coplanar
 * overlap are not intersections; a degenerate face can cut and cannot be cut.  between != 0: only pairs with group[f] != group[g]
 * count (group [n_faces] u8; may be NULL otherwise).  Candidates come from arah_mesh_index_build over the quantised soup, inside
 * the scratch.
 *   hits        [n_faces] i32: the faces each face intersects
 *   vert_hit    [n_verts] u8: 1 for every corner of a face with hits > 0
 *   pair_start  [n_faces + 1] i32, pairs [max_pairs][2] i32: the pairs f < g ordered by f, then g; pair_start is exact, pairs holds
 *               the first max_pairs of them and zero rows behind them (may be NULL for max_pairs = 0)
 *   counts      DEVICE int32 [5]: pairs, faces hit, vertices hit, void faces, pairs written.  More than 2^31 - 1 pairs: counts[0] =
 *               pair_start[n_faces] = -1, no pair is written and the rest of pair_start means nothing
 *   tested      DEVICE int64 or NULL: pairs that reached the six tests, both sides counted (a figure for benchmarks)
 * Integer atomics only, on sums; the result is unique.  0 <= n_faces <= 2^26, 0 <= n_verts, max_pairs <= INT32_MAX, else
 * ARAH_E_BADARG, as for a missing pointer, a quantisation that is not finite or a scratch that is not 256-byte aligned.  scratch:
 * arah_mesh_intersections_scratch_bytes(n_verts, n_faces, max_pairs) device bytes (0 for such sizes).  n_faces = 0 still writes
 * counts and pair_start.  No host synchronisation, no allocation. */
size_t arah_mesh_intersections_scratch_bytes(int64_t n_verts, int64_t n_faces, int64_t max_pairs);
int arah_mesh_intersections(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const uint8_t* group,
                            int32_t between, const float h_origin[3], double scale, int64_t max_pairs, int32_t* hits, uint8_t* vert_hit,
                            int32_t* pair_start, int32_t* pairs, int32_t* counts, int64_t* tested, void* scratch, size_t scratch_bytes,
                            void* stream);

/* Rays against the indexed soup (csrc/meshray.hpp; no reference counterpart).  index / tris: as for arah_mesh_closest, the index
 * is only read.  origins, dirs [R,3] f32 (dirs need not be unit: t is in units of |d|).  The rule per ray and face is Woop, Benthin
 * and Wald's watertight test in float64 on the float32 inputs, every operation rounded on its own (meshing.mesh_raycast states it
 * line by line): a hit is accepted when t is finite, t_min <= t <= t_max, and the point bary . corners lies on the ray at t within
 * 2^-26 of the largest coordinate magnitude of the origin and the face (a ray in a face's plane, whose det is rounding noise, is a
 * miss); cull 0 none, 1 back (drops det < 0: the ray runs along the face's normal (b-a)x(c-a)), 2 front (drops det > 0).
 *   mode 0  first hit: t [R] f64, face [R] i32, bary [R,3] f64 = the lexicographic minimum of (t, face) over the accepted faces,
 *           bit-equal to the brute-force specification whatever the order of the index's references; a miss is t +inf, face -1,
 *           bary 0.  `hit` is not touched (may be NULL).
 *   mode 1  any hit: hit [R] u8, 1 when some face is accepted; the walk stops at the first.  t / face / bary are not touched.
 *   arah_mesh_raycast_debug: the same with the workgroup size given (64, 128 or 256 threads), for measuring it; the results
 *   do not depend on it.
 * n_rays <= 2^31 - 1 - 256.
 * tested [R] i32 or NULL: ray-triangle tests made.  A ray with a zero or non-finite direction or a non-finite origin, and every
 * ray of an index whose status is 1 (a vertex is not finite), misses.  One thread per ray: the big list, then the cells along
 * the ray with the distance transform as an empty-space skip.  Nothing is allocated, nothing truncated, no host synchronisation. */
int arah_mesh_raycast(const void* index, size_t index_bytes, const float* tris, int32_t n_faces, const float* origins,
                      const float* dirs, int32_t n_rays, double t_min, double t_max, int32_t cull, int32_t mode, double* t,
                      int32_t* face, double* bary, uint8_t* hit, int32_t* tested, void* stream);
int arah_mesh_raycast_debug(const void* index, size_t index_bytes, const float* tris, int32_t n_faces, const float* origins,
                            const float* dirs, int32_t n_rays, double t_min, double t_max, int32_t cull, int32_t mode,
                            int32_t workgroup, double* t, int32_t* face, double* bary, uint8_t* hit, int32_t* tested, void* stream);

/* Exact nearest point of a large cloud, and the per-side reduction of the geometry scores over meshes and clouds
 * (csrc/pointdist.hpp; no reference counterpart).  points [n,3] f32; a point with a non-finite coordinate is skipped by the
 * build and is never anyone's neighbour.
 *   arah_point_index_build  a uniform grid over the bounding box of the finite points, each point recorded in its one cell,
 *                           with the distance transform of the occupied cells, into the caller's `index` buffer
 *                           (arah_point_index_bytes(n) bytes, 256-byte aligned).  The cell size is derived from the measured
 *                           occupancy of a coarse lattice at two scales (the cloud's box-counting dimension) under a budget
 *                           of 8 cells per point; the buffer's size is fixed by n alone.  Nothing is truncated.
 *   arah_point_nearest      queries [Q,3] f32 -> d2 [Q] f64 (dx dx + dy dy + dz dz of the float64 differences), nearest [Q]
 *                           i32 (index into the cloud), tested [Q] i32 or NULL (point tests the query made): the
 *                           lexicographic minimum of (d2, index), whatever the order of the build.  A non-finite query gives
 *                           d2 NaN, nearest -1; a cloud without a finite point gives d2 +inf, nearest -1.  `cloud` / n_cloud:
 *                           what the index was built from.
 *   arah_sample_scores      one side of the scores: d2 [n] f64 of its samples; optionally sample_normals [n,3] f64 with
 *                           other_normals [n_other,3] f64 and idx [n] i32 into them (both NULL: no normal term; an idx outside
 *                           [0, n_other) gives a NaN term); thr2 [T] DEVICE f64 squared thresholds, T <= 16 -> sums [6] DEVICE
 *                           doubles: sum d, sum d^2, sum |n . n'|, max d, samples in the distance sums, samples in the normal
 *                           sum; within [T] DEVICE i64: samples with d2 <= thr2[t], counted in integers.  Sums run in index
 *                           order (no floating-point atomics).  scratch: arah_sample_scores_bytes(n) bytes, 8-byte aligned.
 * No host synchronisation anywhere. */
size_t arah_point_index_bytes(int32_t n_points);
int arah_point_index_build(const float* points, int32_t n_points, void* index, size_t index_bytes, void* stream);
int arah_point_nearest(const void* index, size_t index_bytes, const float* cloud, int32_t n_cloud, const float* queries,
                       int32_t n_queries, double* d2, int32_t* nearest, int32_t* tested, void* stream);
size_t arah_sample_scores_bytes(int32_t n);
int arah_sample_scores(const double* d2, int32_t n, const double* sample_normals, const double* other_normals, int32_t n_other,
                       const int32_t* idx, const double* thr2, int32_t n_thresholds, double* sums, int64_t* within, void* scratch,
                       size_t scratch_bytes, void* stream);

/* ---- the hot path ----------------------------------------------------------------------- */
/* rays: cam_loc [n_cams,3], ray r belongs to camera r / rays_per_cam; dirs [N,3]; near_far [N,2].
 * root_find_all: 0 = joint root find on the non-diverged rays (eval), 1 = on every ray (training, RT:249).
 * -> points_hat_norm [N,3], T [N,16], conv [N], start [N], end [N]   (RT:283-296) */
int arah_trace(const ArahFrame* h_frame, const float* cam_loc, int32_t rays_per_cam, const float* dirs,
               const float* near_far, int32_t n_rays, int32_t root_find_all, float* points_hat_norm, float* T,
               uint8_t* conv, float* start, float* end, void* workspace, size_t workspace_bytes, void* stream);
/* rand_steps [N,S], rand_near [N,near+1], rand_far [N,far]: uniform [0,1) draws for the stratified jitter of
 * training mode (perturb_z_vals, RT:298-311, in the order the reference draws them); all NULL = eval mode.
 * -> z [N,S], pts [N,S,3] normalised canonical, T [N,S,16], mask [N,S]   (RT:380, 549-555) */
int arah_sample_canonicalize(const ArahFrame* h_frame, const ArahSampling* h_cfg, const float* cam_loc,
                             int32_t rays_per_cam, const float* dirs, const float* near_far,
                             const uint8_t* conv, const float* start, const float* end, int32_t n_rays,
                             const float* rand_steps, const float* rand_near, const float* rand_far,
                             float* z, float* pts, float* T, uint8_t* mask, void* workspace,
                             size_t workspace_bytes, void* stream);
/* -> rgb [N,3], acc [N], vol_mask [N]   (IDR:148, 225-230, 261-396) */
int arah_shade_composite(const ArahFrame* h_frame, const ArahSampling* h_cfg, const float* dirs,
                         const float* z, const float* pts, const float* T, const uint8_t* mask,
                         int32_t n_rays, float* rgb, float* acc, uint8_t* vol_mask, void* workspace,
                         size_t workspace_bytes, void* stream);
/* Per-sample half of loop D as a seam of its own (IDR:291-368 before the compositing): the SHIPPED shading kernel -- on a
 * split-engine frame the bf16 x 3 normal sweep and colour MLP (shade_engine = ARAH_SHADE_ENGINE_FP32: the fp32 MFMA), on an fp32 frame the
 * exact engine -- on n normalised canonical points with their own blended transforms T [n,16] and ray directions dirs [n,3].
 * -> rgbs [n,4] = {rgb, VolSDF density}, sdfn [n,4] = {sdf (normalised units), d sdf / d x_norm}.  Needs a workspace of
 * arah_workspace_bytes(n, 1). */
int arah_shade_points(const ArahFrame* h_frame, const float* x_norm, const float* T, const float* dirs, int32_t n_pts,
                      int32_t cano_view_dirs, int32_t shade_engine, float* rgbs, float* sdfn, void* workspace,
                      size_t workspace_bytes, void* stream);
/* whole eval forward.  pose34 = DEVICE [3][4] world->camera (R|t), read by the last kernel only (no host copy of
 * the pose, no stream drain).  Any of the optional outputs may be NULL, then they live in the workspace.
 * -> rgb [N,3], points_cam [N,3], vol_mask [N] */
int arah_render(const ArahFrame* h_frame, const ArahSampling* h_cfg, const float* cam_loc,
                int32_t rays_per_cam, const float* dirs, const float* near_far, const float* pose34,
                int32_t n_rays, float* rgb, float* points_cam, uint8_t* vol_mask, float* acc,
                float* dists, uint8_t* surface_conv, void* workspace, size_t workspace_bytes,
                void* stream);

/* arah_render plus a normal map and a depth map, composited with the weights w_i of the rgb.  For every valid sample i that
 * is shaded, n_i = normalize(T_i[:3,:3] . d sdf / d x_norm (x_norm_i)): the posed (world-frame) unit normal, pointing towards
 * positive sdf (the normal the reference gives the colour network with cano_view_dirs = False, IDR:338-340).  Per ray:
 *   normal_world [N,3] = sum_i w_i n_i   (not renormalised: |normal_world| <= acc)
 *   depth [N]          = sum_i w_i z_i   (z: the ray parameter of the samples, the units of `dists`)
 *   acc [N]            = sum_i w_i       (the existing output)
 * 0 on rays without valid samples.  Samples that are not shaded have weight exactly 0 and contribute +0; the tiered path
 * gives the untiered path's maps bit for bit, and rgb, points_cam, vol_mask, acc, dists, surface_conv are arah_render's bit
 * for bit.  maps_buf: a caller buffer of arah_render_maps_bytes(n_rays, n_steps) bytes (16 bytes per sample: the per-sample
 * normals), next to the workspace of arah_workspace_bytes. */
size_t arah_render_maps_bytes(int32_t n_rays, int32_t n_steps);
int arah_render_maps(const ArahFrame* h_frame, const ArahSampling* h_cfg, const float* cam_loc,
                     int32_t rays_per_cam, const float* dirs, const float* near_far, const float* pose34,
                     int32_t n_rays, float* rgb, float* points_cam, uint8_t* vol_mask, float* acc,
                     float* dists, uint8_t* surface_conv, float* normal_world, float* depth, void* workspace,
                     size_t workspace_bytes, void* maps_buf, size_t maps_buf_bytes, void* stream);

/* ---- tiered evaluation (csrc/tier.hpp) --------------------------------------------------------- */
/* The reference evaluates every depth sample of every ray (ray_tracing.py:313-380 -> search_canonical_corr,
 * implicit_differentiable_renderer.py:336-368); a sample whose canonical point lies outside {sdf <= 18 beta} has density
 * exactly +0 there.  arah_prepare_occupancy voxelises the POSED image of that set for a prepared frame (SDF lattice of
 * [-1.5,1.5]^3, refined where the band can be, skinned forward with the skinning MLP, dilated by the lattice's reach) into a
 * caller buffer of arah_occupancy_bytes() bytes; ArahSampling.occupancy hands it to arah_render. */
size_t arah_occupancy_bytes(void);
int arah_prepare_occupancy(const ArahFrame* h_frame, void* occ_buf, size_t occ_bytes, void* workspace,
                           size_t workspace_bytes, void* stream);
/* the 16 words at the head of an occupancy buffer: origin[3], voxel, 1/voxel, dims[3], n_vox, valid, n_cells, n_fine,
 * n_selected, overflow, band (m), steepest measured stretch of the forward skinning between adjacent selected lattice points;
 * synchronises the stream */
int arah_occupancy_info(const void* occ_buf, int32_t* h_out16, void* stream);
/* after an arah_render on this workspace: ray_tier [N] (0 certified zero, 1 surface ray, 2 promoted; tiered path only) and
 * ray_sigma_pos [N] (1: some valid sample of the ray has density > 0); device pointers, either may be NULL */
int arah_tier_debug(void* workspace, size_t workspace_bytes, int32_t n_rays, int32_t n_steps, uint8_t* ray_tier,
                    uint8_t* ray_sigma_pos, void* stream);

/* Audit of the certificate (csrc/tier.hpp).  The tiers rest on assumptions the kernels cannot prove (the SDF's and the forward
 * skinning's Lipschitz constants over a lattice cell, the fat body inside [-1.5, 1.5]^3); arah_tier_audit re-examines, with the
 * production kernels, a deterministic sample of what the LAST tiered arah_render on `workspace` skipped:
 *   A  certified samples that converged (phase 1's witnesses, every phase-2 sample): density evaluated; violation: not +0;
 *   B  samples never evaluated (rays not promoted): nearest vertex, loop C, density; violation: converged with density not +0;
 *   C  rays kept out of loops A+B (their segment misses the bitmap): traced again; violation: the ray converges.
 * Ordering rule: enqueue it on the render's stream right behind that arah_render, before anything else uses the workspace or
 * the occupancy buffer, with the same h_cfg (occupancy included) and ray arguments.  It reads the workspace and never writes
 * it (outputs, debug arrays and ArahCounters stay as the render left them); all of its own state lives in audit_buf
 * (arah_tier_audit_bytes(n_rays, n_steps) bytes, 256-byte aligned: about one more workspace), the result at its head.
 * Selection: sample q = ray * n_steps + s (classes A, B) and ray index (class C) are examined when
 *   (h(x, seed) & ((1 << rate_log2) - 1)) == 0,   h(x, seed) = fmix32(x * 0x9E3779B1 + seed)   (uint32 arithmetic),
 *   fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16  (MurmurHash3's finaliser);
 * rate_log2 = 0 examines everything skipped.  The audit detects violations; with rate_log2 > 0 it cannot prove their absence. */
typedef struct ArahTierAudit {
    uint64_t a_examined, a_violations;
    uint64_t b_examined, b_converged, b_violations;
    uint64_t c_examined, c_violations;
    uint64_t n_first;             /* entries of first_index / first_class written: min(8, all violations), in no particular order */
    int64_t first_index[8];       /* sample index ray * n_steps + s (classes A, B) or ray index (class C) */
    int32_t first_class[8];       /* 0 = A, 1 = B, 2 = C */
    float min_ratio;              /* smallest metric sdf / beta over the examined converged A / B samples (+inf: none); the
                                     certificate holds with room while this stays above 17.33 */
    int32_t rate_log2;
    uint32_t seed;
    int32_t reserved;
} ArahTierAudit;
size_t arah_tier_audit_bytes(int32_t n_rays, int32_t n_steps);
int arah_tier_audit(const ArahFrame* h_frame, const ArahSampling* h_cfg, const float* cam_loc, int32_t rays_per_cam,
                    const float* dirs, const float* near_far, int32_t n_rays, int32_t rate_log2, uint32_t seed, void* audit_buf,
                    size_t audit_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* tests: per sample [N,S] the audit's verdict (1 class A, 2 class B, | 4 converged, | 8 violation; 0 not examined) and per
 * ray [N] (1 class C examined, 3 examined and converged); device pointers, either may be NULL */
int arah_tier_audit_debug(const void* audit_buf, size_t audit_bytes, int32_t n_rays, int32_t n_steps, uint8_t* sample_tag,
                          uint8_t* ray_tag, void* stream);
/* tests only: damage a certificate on purpose -- unmark the voxels of an occupancy buffer whose centres lie in the posed-space
 * box [h_lo, h_hi] (metres, 3 floats each, host) and recompute its distance transform */
int arah_occupancy_clear_box(void* occ_buf, const float* h_lo, const float* h_hi, void* stream);

/* tests: the per-sample arrays of the workspace's last arah_render, copied device to device (any pointer may be NULL):
 * z [N,S], pts [N,S,3] normalised canonical, T [N,S,16], mask [N,S], shaded [N,S,4] = {rgb, density}, state [N,S] */
int arah_debug_samples(void* workspace, size_t workspace_bytes, int32_t n_rays, int32_t n_steps, float* z, float* pts,
                       float* T, uint8_t* mask, float* shaded, uint8_t* state, void* stream);

/* tests: two helper kernels of the frame exist twice, as a serial specification (variant 0) and as the cooperative kernel the
 * frame runs (variant 1); both entries are pure functions of the caller's device buffers, and the variants agree bit for bit.
 *
 * arah_sample_depths_debug: the eval-mode (no jitter) depth samples of n rays -> z [n, n_steps], mask [n, n_steps];
 * near_far [n,2], conv [n], start [n], end [n] as the tracer leaves them, lin_* as in ArahSampling.  Variant 1 is the function
 * the tiered frame's classifier computes its depths with.
 *
 * arah_cell_clusters_debug: the per-cell candidate lists of the nearest-vertex search -> cells [n_cells][64] (byte 0: the
 * count, or 255 when more than 63 clusters qualify; then the cluster ids in the order of their lower bounds).  grid and spheres
 * are device pointers into a body buffer (arah_prepare_body; byte offsets ARAH_BODY_OFF_*) or buffers of the same layout. */
#define ARAH_BODY_OFF_SPHERES 114688u /* [256][4] float: centre, radius */
#define ARAH_BODY_OFF_GRID 118784u    /* origin[3], h, 1/h (float) | dims[3], n_cells, n_clusters, pad[2] (int32) */
#define ARAH_BODY_OFF_CELLS 119040u   /* [<= 65536][64] uint8 */
int arah_sample_depths_debug(int32_t variant, int32_t n_rays, int32_t n_steps, int32_t n_near, int32_t n_far,
                             const float* near_far, const uint8_t* conv, const float* start, const float* end,
                             const float* lin_steps, const float* lin_near, const float* lin_far, float* z, uint8_t* mask,
                             void* stream);
int arah_cell_clusters_debug(int32_t variant, const void* grid, const float* spheres, uint8_t* cells, void* stream);

/* ---- posed-space queries (csrc/posed.hpp) ---------------------------------------------------------------------------------- */
/* The value of the lattice / the sdf of a certified point: any positive value would do (marching cubes at level 0 only reads signs
 * there); metres. */
#define ARAH_POSED_FILL 1.0f
/* Per world-space point, what the eval forward computes for a depth sample at that position: nearest SMPL vertex + inverse LBS
 * (ray_tracing.py:408-421; exact for every point: outside the nearest-vertex grid's box the search walks every cluster), Broyden
 * on LBS(x_hat) - (x - trans) with the solver ARAH_CANON_KERNEL selects (wave | tile | wave_l2, read once per process), the SDF
 * trunk at the normalised solution.  pts [P,3] world metres (finite) ->
 *   sdf [P]          metres, sdf_norm / 2 * 1.1 * (coord_max - coord_min)   (implicit_differentiable_renderer.py:359)
 *   x_hat_norm [P,3] the normalised canonical solution (or NULL)
 *   T [P,16]         the blended forward transform the solver returns (or NULL)
 *   normal [P,3]     normalize(T[:3,:3] . d sdf / d x_norm), the posed normal of arah_render_maps (or NULL: no gradient sweep)
 *   weights [P,24]   the skinning MLP's weights at x_hat (or NULL)
 *   state [P]        0: not converged (values of the solver's best iterate), 1: converged, 2: skipped -- occ_buf (arah_prepare_occupancy
 *                    of THIS frame, or NULL) certifies that the point is outside the posed fat body (sigma = +0 for a sample there):
 *                    only sdf is written, +ARAH_POSED_FILL, the other outputs are left untouched.
 * Every field of an evaluated point is bit-equal whether or not occ_buf is passed, whatever the list's length and the point's
 * position in it.  buf: arah_query_posed_bytes(n_pts) bytes (256-byte aligned); long lists run in passes of a fixed size, so the
 * buffer stays below ~130 MB.  No host synchronisation. */
size_t arah_query_posed_bytes(int32_t n_pts);
int arah_query_posed(const ArahFrame* h_frame, const void* occ_buf, const float* pts, int32_t n_pts, float* sdf, float* x_hat_norm,
                     float* T, float* normal, float* weights, uint8_t* state, void* buf, size_t buf_bytes, void* stream);
/* The posed SDF on the n^3 lattice of a world-space cube: point (ix, iy, iz) at origin + (i / (n - 1)) side, sdf[(ix*n + iy)*n + iz]
 * in metres (arah_marching_cubes' output maps to world coordinates by x_world = origin + (x + 1) / 2 * side).
 * box: DEVICE [4] origin xyz, side; NULL = the cube around the bounding box of occ_buf's MARKED voxels plus one voxel (the
 * whole bitmap box if nothing is marked or the bitmap is invalid).  box_out: DEVICE [4], the cube used.
 * Value rule: converged points take their sdf, unconverged and skipped points +ARAH_POSED_FILL.
 * band = 1 (needs occ_buf): a point is evaluated only when it shares a lattice cell with a lattice point in a marked voxel (outside
 * the bitmap's box counts as marked); the others are skipped.  When the certificate holds, every corner of every cell whose values
 * change sign is evaluated, so arah_marching_cubes gives band = 0's triangle soup bit for bit.
 * counts: DEVICE [3] int32 evaluated, converged, skipped.  buf: arah_sdf_grid_posed_bytes(n_side) bytes; 2 <= n_side <= 1024. */
size_t arah_sdf_grid_posed_bytes(int32_t n_side);
int arah_sdf_grid_posed(const ArahFrame* h_frame, const void* occ_buf, const float* box, int32_t n_side, int32_t band, float* sdf,
                        float* box_out, int32_t* counts, void* buf, size_t buf_bytes, void* stream);

/* ---- containment against large meshes, occupancy grids (csrc/meshcontains.hpp) ---------------------------------------------- */
/* Is a point inside a mesh: libmesh's check_mesh_contains (im2mesh/utils/libmesh/inside_mesh.py) with its TriangleHash restated on
 * the device; the rule is meshing.mesh_contains and every result equals it bit for bit.  verts [V,3] float, faces [F,3] int32,
 * 0 <= F <= 2^28, 2 <= resolution <= 4096, otherwise ARAH_E_BADARG without a launch and a size of 0.  A mesh without faces, with
 * a face id outside [0, V), a non-finite used vertex or no extent on an axis is DEGENERATE: every point is outside.
 *
 * The index is built in two calls because its number of references is data-dependent:
 *   arah_contains_index_count   bounds, per-triangle records and cell rectangles, per-cell counts and their scan into `index`
 *                               (arah_contains_index_bytes(F, resolution) device bytes, 256-byte aligned).  The first 256 bytes are
 *                               the header: 7 doubles scale[3], translate[3], resolution | int64 n_refs | int32 n_faces, resolution,
 *                               valid, status (bit 0: n_refs > INT32_MAX) | uint32 n_med, n_huge.
 *   the caller reads n_refs from the header (the index's one host synchronisation) and allocates refs [n_refs] int32;
 *   arah_contains_index_fill    the triangle ids of every cell into refs (cell c: refs[start[c] .. start[c+1])).  ARAH_E_OVERFLOW for
 *                               n_refs > INT32_MAX; n_refs = 0: nothing to do, refs may be NULL.
 * The order of the ids inside a cell is unspecified; the answers do not depend on it.
 *
 * arah_mesh_contains: pts [P,3] float32 or float64 -> inside [P] u8, ambiguous [P] u8 (or NULL), tested [P] int32 candidates (or
 * NULL).  One lane per point; rows past P are never written; P = 0 is legal.  An n_refs that is not the header's: every point is
 * outside.  No host synchronisation.
 *
 * arah_mesh_contains_grid: the lattice xs[nx] x ys[ny] x zs[nz] (float32) -> occupancy [nx][ny][nz] u8 in C order, equal to
 * arah_mesh_contains on the meshgrid(indexing="ij") bit for bit; ambiguous: DEVICE uint64, the number of ambiguous lattice points
 * (or NULL).  nx, ny, nz >= 1, nx ny <= INT32_MAX, nx ny nz <= 2^33.  No host synchronisation. */
size_t arah_contains_index_bytes(int32_t n_faces, int32_t resolution);
int arah_contains_index_count(const float* verts, int32_t n_verts, const int32_t* faces, int32_t n_faces, int32_t resolution,
                              void* index, size_t index_bytes, void* stream);
int arah_contains_index_fill(void* index, size_t index_bytes, int32_t n_faces, int32_t resolution, int32_t* refs, int64_t n_refs,
                             void* stream);
int arah_mesh_contains(const void* index, size_t index_bytes, int32_t n_faces, int32_t resolution, const int32_t* refs, int64_t n_refs,
                       const void* pts, int32_t pts_are_f64, int32_t n_pts, uint8_t* inside, uint8_t* ambiguous, int32_t* tested,
                       void* stream);
int arah_mesh_contains_grid(const void* index, size_t index_bytes, int32_t n_faces, int32_t resolution, const int32_t* refs,
                            int64_t n_refs, const float* xs, int32_t nx, const float* ys, int32_t ny, const float* zs, int32_t nz,
                            uint8_t* occupancy, uint64_t* ambiguous, void* stream);

/* ---- the truncated signed distance field of a soup on a lattice (csrc/meshsdf.hpp; no reference counterpart) ------------------- */
/* The distance of every node of the lattice xs[nx] x ys[ny] x zs[nz] (float32, each axis strictly ascending: the convention of
 * arah_mesh_contains_grid) to the soup tris [F,3,3] float32, cut off at trunc; the rule is meshing.mesh_sdf_grid, and d2 / face
 * equal it bit for bit.  All arrays [nx][ny][nz] in C order:
 *   d2        f64: the squared distance to the closest triangle (arah_mesh_closest's arithmetic), +inf where it exceeds
 *             (double)trunc^2 -- the node is outside the BAND.  trunc = +inf cuts nothing off; trunc = 0 keeps the nodes on the surface
 *   face      i32 or NULL: the lowest id among the triangles at that distance, -1 outside the band (asking for it walks the
 *             band a second time)
 *   sdf       f32 or NULL: (occupancy ? -1 : +1) * min(sqrt(d2), trunc) in float64, rounded once -- meshing.signed_distance
 *   occupancy u8 or NULL: as arah_mesh_contains_grid writes it on the same lattice; NULL counts every node as outside
 *   info      DEVICE int32 [8], 8-byte aligned: [0] nodes in the band, [1] status, [2..3] point-triangle tests made (one uint64), [4..7] triangles
 *             of the size classes lane / wave / workgroup / several workgroups (a triangle whose dilated box holds no node is in none)
 * status 1: some vertex is not finite; then d2 is NaN and face -1 everywhere, as arah_mesh_closest answers.  A node with a
 * coordinate that is not finite gets NaN / -1 too.  F = 0: +inf / -1 everywhere.
 * The work follows the band: each triangle visits the nodes inside its bounding box dilated by trunc (a conservative superset of
 * the nodes within trunc of it).  Integer atomics only: the result does not depend on the order of arrival.  Nothing is
 * truncated.  No host synchronisation.  scratch: arah_mesh_sdf_grid_bytes(F, nx, ny, nz) device bytes, 256-byte aligned; 0 for
 * a size that is negative or too large.  0 <= F <= 2^26.  ARAH_E_OVERFLOW when nx ny nz does not fit an int32, ARAH_E_BADARG for
 * a trunc that is negative or NaN. */
size_t arah_mesh_sdf_grid_bytes(int64_t n_faces, int64_t nx, int64_t ny, int64_t nz);
int arah_mesh_sdf_grid(const float* tris, int32_t n_faces, const float* xs, int32_t nx, const float* ys, int32_t ny, const float* zs,
                       int32_t nz, float trunc, const uint8_t* occupancy, double* d2, int32_t* face, float* sdf, int32_t* info,
                       void* scratch, size_t scratch_bytes, void* stream);

/* ---- generalized winding numbers (csrc/meshwinding.hpp; no reference counterpart) ------------------------------------------------ */
/* The generalized winding number of points against a triangle mesh, evaluated hierarchically (Barill et al. 2018, first order):
 * exact solid angles (Van Oosterom & Strackee) for the triangles of near leaves, one dipole for a far cluster.  The rule is
 * meshing.winding_tree / meshing.mesh_winding; float64 throughout.  Every integer table equals the rule's, every float table, every
 * near / far decision and every dipole term equal it bit for bit; only atan2 may differ, by its last bits.  verts [V,3] float, faces
 * [F,3] int32, 0 <= F <= 2^28, depth in [0, 7] or -1 for the rule of meshing.winding_depth; otherwise ARAH_E_BADARG without a launch
 * and a size of 0.
 *
 * The index is built in two calls because its number of nodes is data-dependent:
 *   arah_winding_index_count   the cube, the leaf keys, the list ordered by (key, face id) -> order [F] int32 and tris [F,3,3] float32
 *                              (the corners in list order), and the preorder numbering into `index` (arah_winding_index_bytes(F,
 *                              depth) device bytes, 256-byte aligned).  The first 256 bytes are the header: 5 doubles lo[3], side,
 *                              volume | int64 n_nodes | int32 n_faces, depth, valid (every used vertex finite), status (bit 0: a face
 *                              id outside [0, V); bit 1: at depth > 0 a leaf cell holds more than 2^15 faces -- ranking a cell's
 *                              faces is quadratic in the cell, so that cell is left in the order of arrival, valid is 0 and every
 *                              winding number NaN), orient (+1 / -1, the sign of the signed volume; +1 for 0).
 *   the caller reads n_nodes from the header (the index's one host synchronisation) and allocates node_i [n_nodes][4] int32
 *   (first, count, level, skip) and node_f [n_nodes][8] float64 (centroid xyz, radius, area vector xyz, area);
 *   arah_winding_index_fill    writes the two tables.  ARAH_E_OVERFLOW for n_nodes > INT32_MAX; n_nodes = 0: nothing to do.
 *
 * arah_mesh_winding: pts [P,3] float32 -> w [P] f64, and on request inside [P] u8 (orient * w >= 0.5; a NaN is outside), n_exact [P]
 * int32 (triangles summed exactly) and n_far [P] int32 (dipoles), each or NULL.  accuracy >= 1, +inf for the exact sum, else
 * ARAH_E_BADARG.  One lane per point, each point's sum in the rule's order; no atomics.  A mesh with a vertex that is not finite:
 * w = NaN.  F = 0: w = 0.  P = 0 is legal.  No host synchronisation.
 *
 * arah_mesh_winding_grid: the lattice xs[nx] x ys[ny] x zs[nz] (float32), all outputs [nx][ny][nz] in C order, equal to
 * arah_mesh_winding on the meshgrid(indexing="ij") bit for bit.  ARAH_E_OVERFLOW when nx ny nz does not fit an int32. */
size_t arah_winding_index_bytes(int32_t n_faces, int32_t depth);
int arah_winding_index_count(const float* verts, int32_t n_verts, const int32_t* faces, int32_t n_faces, int32_t depth, void* index,
                             size_t index_bytes, int32_t* order, float* tris, void* stream);
int arah_winding_index_fill(const void* index, size_t index_bytes, int32_t n_faces, int32_t depth, const float* tris, int32_t* node_i,
                            double* node_f, int64_t n_nodes, void* stream);
int arah_mesh_winding(const void* index, size_t index_bytes, int32_t n_faces, int32_t depth, const float* tris, const int32_t* node_i,
                      const double* node_f, int64_t n_nodes, const float* pts, int32_t n_pts, double accuracy, double* w,
                      uint8_t* inside, int32_t* n_exact, int32_t* n_far, void* stream);
int arah_mesh_winding_grid(const void* index, size_t index_bytes, int32_t n_faces, int32_t depth, const float* tris,
                           const int32_t* node_i, const double* node_f, int64_t n_nodes, const float* xs, int32_t nx, const float* ys,
                           int32_t ny, const float* zs, int32_t nz, double accuracy, double* w, uint8_t* inside, int32_t* n_exact,
                           int32_t* n_far, void* stream);

/* name of the dominant kernel, for profilers */
const char* arah_dominant_kernel(void);
#ifdef __cplusplus
}
#endif
#endif /* ARAH_HIP_H */
