/*
 * mnrf.h -- C ABI of the MI355X-native Mirror-NeRF rendering hot path.
 *
 * The reference has no C/FFI boundary on this path: its boundary is two Python
 * call signatures,
 *     render_rays(models, embeddings, rays, N_samples, use_disp, perturb, noise_std,
 *                 N_importance, chunk, white_back, test_time, **kwargs)   models/rendering.py:54-67
 *     MirrorNeRF.forward(x, compute_normal, sigma_only, embedding_xyz, ...)  models/mirror_nerf.py:101-112
 * which `mirror_nerf_amd/rendering.py` and `mirror_nerf_amd/mirror_nerf.py` keep.
 * Those Python shims do no arithmetic; every number is produced by the entry
 * points below (libmnrf_hip.so), which take plain device pointers and sizes.
 *
 * Conventions
 *   - all pointers are DEVICE pointers to fp32 unless stated; the caller owns every
 *     buffer and the library never allocates device memory.  A packed weight image is
 *     read-write: its last 19 words are device state of the launches that use it (a
 *     {value, done} pair of the training backward's single-launch reductions, 16 counters
 *     of the field kernels' dynamic tile queue -- all zero between launches -- and the
 *     range-guard word below); mnrf_pack_weights zeroes them.  Hence `float* packed`, not const, in every entry
 *     point that launches on an image: an image must not live in read-only or IPC-shared memory;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued, never synchronised;
 *   - return value 0 = ok, negative = error (see mnrf_last_error()); nothing throws;
 *   - re-entrant; no global stream or global device state (host side: a cached CU count
 *     per device and a rotating index into the 8 counter pairs of an image -- at most 8
 *     tile-queue launches that share one image may be in flight on different streams);
 *     every launch is capturable in a hipGraph.
 *   - the field architecture is the reference default (train.py:44-66): D=8, W=256,
 *     skip at layer 5, Embedding(10) for xyz (63 ch), Embedding(4) for dir (27 ch),
 *     normal_net and is_mirror_net present.
 */
#ifndef MNRF_H
#define MNRF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Marks a single-level pointer parameter as HOST memory, read (or written) during the call; every unmarked one is device memory
 * (or `void* stream`, or an argument struct).  `T* const*` parameters are always host arrays of device pointers and carry no
 * marker.  Expands to nothing: it is what the Python binding (mirror_nerf_amd/_abi.py) types the argument from. */
#define MNRF_HOST

#define MNRF_OK 0
#define MNRF_ERR_ARG (-1)      /* bad argument (null pointer, size, flag combination) */
#define MNRF_ERR_LAUNCH (-2)   /* HIP reported an error at launch */
#define MNRF_ERR_UNSUPPORTED (-3)

/* number of parameter tensors of one MirrorNeRF in state_dict order
 * (xyz_encoding_{1..8}.0.{weight,bias}, xyz_encoding_final, dir_encoding.0, sigma,
 *  rgb.0, normal_net.{0,1}, is_mirror_net.{0,2});  utils/__init__.py:109-136 */
#define MNRF_N_PARAMS 32

/* flags of mnrf_field_forward */
#define MNRF_SIGMA_ONLY 1u     /* stop after sigma (rendering.py:139-150) */
#define MNRF_GRAD_NORMAL 2u    /* also emit normal = l2n(-d sigma/d xyz) (mirror_nerf.py:136-146) */
#define MNRF_SPLIT_F16 4u      /* evaluate the Linears on the f16 matrix pipe with every fp32 operand carried as a
                                  hi/lo f16 pair (3 MFMAs per product block, fp32 accumulation; ~2^-20 relative per
                                  product instead of the bit-exact fp32 fmaf chain of the default) */

#define MNRF_TCNN_GRAD_F16 16u  /* mnrf_tcnn_backward: the levels without private copies accumulate their table gradient scaled by 2^10 in
                                  half2 with ONE packed atomic per entry (global_atomic_pk_add_f16) instead of two fp32 atomics --
                                  tinycudann's gradient precision (models/mirror_nerf_tcnn.py:36-49 under train.py:586); the
                                  workspace then has mnrf_tcnn_backward_workspace_floats2() floats */
#define MNRF_TCNN_GRAD_FIXED 512u /* mnrf_tcnn_backward: the levels without private copies accumulate both features of a table entry with ONE
                                  64-bit integer atomic (two 32-bit fixed-point halves under a per-level power-of-two scale taken
                                  from the step's own sum of gradient magnitudes, under which no entry can overflow; exact integer
                                  sums, order-independent; step ~2^-16 of a level's largest contribution); the scatter runs as a second
                                  launch over dL/d encoding planes.  Workspace: mnrf_tcnn_backward_workspace_floats3() floats, of
                                  which the caller zero-fills the first mnrf_tcnn_backward_workspace_floats().  Ignored together
                                  with MNRF_TCNN_GRAD_F16. */
#define MNRF_TCNN_F16 256u      /* mnrf_tcnn_forward: single-pass f16 MLPs -- operands rounded to f16, ONE MFMA per product, fp32 accumulation:
                                  "fp16 MLP on CDNA4 MFMA" as BASELINE config 5 words it and as the reference computes under
                                  tinycudann / precision=16 (train.py:586); ~1e-3 relative; sigma-only launches then take the matrix pipe too */
#define MNRF_TCNN_TABLE_F16 1024u /* mnrf_tcnn_forward / _backward / _encode_flags: `table` points to HALF2 entries (4 B per entry: tinycudann's
                                  storage, models/gridencoder/grid.py:57-58, mirror_nerf_tcnn.py:39-49; SURVEY 8d prices config 5 at 16 x 8 x 4 =
                                  512 B of gathers per sample) made from the fp32 master table by mnrf_tcnn_table_half; gradients still go
                                  to the fp32 d_table (the master the optimizer steps, as tinycudann keeps fp32 master parameters) */
#define MNRF_TCNN_VALU 8u       /* mnrf_tcnn_forward: evaluate the small MLPs with fp32 FMAs on the VALU, one thread per sample
                                  (the first implementation; default: hi/lo f16 tiles on the matrix pipe, ~1e-6 of it) */

/* gradient steering of the training backward (the reference's --detach_density_* options; values are unaffected) */
#define MNRF_CUT_NORMAL_HEAD 32u   /* mnrf_field_backward: normal_net sees geo_feat.detach() (mirror_nerf.py:154-158) */
#define MNRF_CUT_MIRROR_HEAD 64u   /* mnrf_field_backward: is_mirror_net sees geo_feat.detach() (mirror_nerf.py:169-170) */
#define MNRF_DW_ACCUMULATE 128u     /* mnrf_field_backward: ADD the parameter gradients to d_params instead of overwriting them (a
                                      module evaluated more than once per step -- primary and reflected rays -- then needs
                                      no separate accumulation kernels) */
#define MNRF_DETACH_W_MASK 1       /* mnrf_composite_backward: mirror mask = sum(weights.detach() * is_mirror) (rendering.py:223-226) */
#define MNRF_DETACH_W_NORMAL 2     /* mnrf_composite_backward: the normal outputs use weights.detach() (rendering.py:244-264) */

/* Range guard of the split-f16 arithmetic.  The LAST 32-bit word of a packed weight image (index
 * mnrf_packed_floats() - 1) is a sticky device flag: mnrf_pack_weights clears it, every MNRF_SPLIT_F16 kernel ORs in */
#define MNRF_GUARD_SATURATED 1u    /* an operand of a Linear reached the f16 maximum: hi/lo pairs no longer carry fp32 */
#define MNRF_GUARD_WEIGHT 2u       /* a weight is non-finite or >= 65504 in magnitude (set by mnrf_pack_weights) */
#define MNRF_GUARD_IN_FORWARD 128u       /* with SATURATED, which pass: ... an activation of a forward evaluation */
#define MNRF_GUARD_IN_BACKWARD 256u      /* ... a scaled activation gradient of the training backward (mnrf_field_backward_planes: the
                                            caller may lower the gradient scale instead of leaving the split arithmetic, see its flags) */
#define MNRF_GUARD_IN_SECOND_ORDER 512u  /* ... a scaled tangent or signal of the second-order pass (mnrf_field_backward2*) */
#define MNRF_GUARD_ENC_RANGE 4u    /* a position with |x| >= 64: sin/cos arguments beyond 2^15, outside the fast exact reduction */
/* The fp32 kernels never touch it.  Host policy (mirror_nerf_amd.mirror_nerf.check_guard): read it once per frame /
 * training step; non-zero -> the module is switched to the exact fp32 kernels and the work is repeated. */

const char* mnrf_last_error(void);
int mnrf_version(void);

/* Size in floats of the packed weight image of one model (forward stream, bias block,
 * transposed trunk stream for the density gradient). */
int64_t mnrf_packed_floats(void);

/* Re-lay one model's parameters into the MFMA-fragment order the field kernel streams
 * through LDS.  `params` is a HOST array of MNRF_N_PARAMS device pointers in state_dict
 * order (nn.Linear layout (out,in) row-major, models/mirror_nerf.py:59-99).
 * Replaces: the implicit weight reads of nn.Linear at call time. */
int mnrf_pack_weights(const float* const* params, float* packed, void* stream);
/* The same for n_models models at once (a training step re-packs its coarse and its fine model behind every optimizer step: one
 * launch pair instead of one per model): params = n_models x 32 pointers, model after model; packed = n_models images. */
int mnrf_pack_weights_n(int n_models, const float* const* params, float* const* packed, void* stream);
/* Folded forward stream of n_models packed images (same arguments as mnrf_pack_weights_n): normal_net's two Linears as one map,
 * xyz_encoding_final folded into dir_encoding, formed in fp64 on the GPU.  The full forward-only split launches (mnrf_field_forward
 * with MNRF_SPLIT_F16 and neither MNRF_SIGMA_ONLY nor MNRF_GRAD_NORMAL, mnrf_field_composite_fused) read it: call this after
 * every mnrf_pack_weights* of an image and before its first such launch. */
int mnrf_fold_weights_n(int n_models, const float* const* params, float* const* packed, void* stream);

/* Embedding.forward (models/mirror_nerf.py:20-38): x (n, c) -> out (n, c*(2*n_freqs+1)). */
int mnrf_embed(const float* x, int64_t n, int c, int n_freqs, float* out, void* stream);

/* MirrorNeRF.forward on B samples (models/mirror_nerf.py:101-187).
 * Positions: either `xyz` (B rows, `xyz_stride` floats apart), or -- when xyz is null --
 * generated as o + d*z from `rays` (n_rays, 8) and `z_vals` (n_rays, spr) with B = n_rays*spr
 * (rendering.py:302; separate multiply and add).
 * View encoding: `dir_emb` rows of 27 floats, `dir_stride` floats apart; row index is
 * sample/spr (spr = 1 when every sample carries its own row, as in forward(x)).
 * Outputs may be null when not wanted: sigma (B), rgb (B,3), pred_normal (B,3),
 * is_mirror (B), normal (B,3), geo_feat (B,256). */
int mnrf_field_forward(float* packed, unsigned flags, int64_t B,
                       const float* xyz, int64_t xyz_stride,
                       const float* rays, const float* z_vals, int spr,
                       const float* dir_emb, int64_t dir_stride,
                       float* sigma, float* rgb, float* pred_normal, float* is_mirror,
                       float* normal, float* geo_feat, void* stream);

/* Coarse depths (rendering.py:283-300): z = near*(1-t)+far*t, or in disparity;
 * `z_steps` (n_samples) is torch.linspace(0,1,n) from the host (not recomputed: SURVEY 8a
 * hazard 2); `perturb_rand` (n_rays, n_samples) may be null (perturb == 0). */
int mnrf_sample_coarse(const float* rays, int64_t n_rays, const float* z_steps, int n_samples,
                       int use_disp, float perturb, const float* perturb_rand, float* z_vals,
                       void* stream);

/* Alpha compositing along each ray (rendering.py:181-264, 362-367).
 * Inputs per sample: sigma, z_vals (n_rays, S); optional noise (already scaled by noise_std);
 * optional rgb (.,3), is_mirror, pred_normal (.,3), normal (.,3).
 * Outputs (null = skip): weights (n_rays,S), opacity, rgb_map (.,3), depth, mirror_mask,
 * surf_normal (.,3) [sum w*pred_normal], surf_normal_grad (.,3) [sum w*normal],
 * normal_dif [sum w*|normal-pred_normal|^2], x_surface (.,3) = o + d*depth. */
int mnrf_composite(const float* rays, int64_t n_rays, int S, const float* sigma, const float* z_vals,
                   const float* noise, const float* rgb, const float* is_mirror,
                   const float* pred_normal, const float* normal, int white_back,
                   float* weights, float* opacity, float* rgb_map, float* depth, float* mirror_mask,
                   float* surf_normal, float* surf_normal_grad, float* normal_dif, float* x_surface,
                   void* stream);

/* Hierarchical resampling (rendering.py:7-51, 312-326): inverse-CDF samples from
 * weights[:,1:-1] over the mid-points of z_coarse, merged and sorted with z_coarse.
 * `u`: (n_importance) shared by all rays when u_per_ray == 0 (torch.linspace(0,1,n), det=True)
 * or (n_rays, n_importance) when u_per_ray != 0.  z_fine: (n_rays, S + n_importance). */
int mnrf_sample_fine(const float* z_coarse, const float* weights, int64_t n_rays, int S,
                     const float* u, int u_per_ray, int n_importance, float* z_fine, void* stream);

/* Reflected-ray construction + order-preserving compaction
 * (train.py:192-252, eval.py:336-360, 513-548).
 * mask (n_rays) is the 0/1 (or soft) mirror mask; a ray is selected iff mask != 0 (the
 * `.bool()` of the reference).  compact == 0 keeps all rays (count = n_rays).
 * normal_noise (n_rays,3) may be null (eval.py:506-511 roughness).
 * Writes sec_rays (count, 8) = [x_surface, r, near2, far], index (count) int32 of the source
 * ray, *count (int32, device), and optionally reflect_dir (n_rays, 3) for all rays. */
int mnrf_reflect_compact(const float* rays, const float* x_surface, const float* normal,
                         const float* normal_noise, float noise_std, const float* mask,
                         int64_t n_rays, int compact, float near2, float* sec_rays, int32_t* index,
                         int32_t* count, float* reflect_dir, void* stream);

/* Threshold in place exactly like `m[m>0.5]=1; m[m<0.5]=0` (train.py:165-166, eval.py:305-306)
 * and OR-reduce `m != 0` into *any (int32, device, caller zeroes it). */
int mnrf_threshold_mask(float* mask, int64_t n, int32_t* any, void* stream);

/* Blend (train.py:261-296, eval.py:676-697): out = m*part + (1-m)*base, where part is
 * `sec` scattered through `index` (compacted, rows without a source keep `base`) or `sec`
 * itself (index == null).  Optionally writes reflect_out (n,c) = scattered sec (zeros elsewhere). */
int mnrf_blend_scatter(const float* base, const float* sec, const int32_t* index, int64_t n_sec,
                       const float* mask, int64_t n, int c, float* out, float* reflect_out,
                       void* stream);

/* Scene editing (eval.batched_inference applications, round 7).
 *
 * Place a new axis-aligned planar mirror into one recursion level (eval.py:364-504, app_place_new_mirror).  Per ray of
 * rays (n_rays,8): the intersection x of the ray's line with the plane x = position (axis MNRF_PLANE_X; the rectangle bounds
 * (y, z)) or y = position (MNRF_PLANE_Y; bounds (x, z)), written `t = (position - o_a) / d_a`, `t * d_b + o_b` as the
 * reference does.  A ray is inside the rectangle when `!(u < rect_u0 || w < rect_w0 || u > rect_u1 || w > rect_w1)` (a NaN
 * coordinate counts as inside); those rays get normal (n_rays,3) = (normal_x, normal_y, normal_z) in place.  The ones whose
 * intersection also lies ahead of the origin (`sum((x - o) * d) > 0`) and is not behind the foreground
 * (`!(|o - x| > depth && depth > near)`, depth of the level before this call, near = the global hyper-parameter) hit the new
 * mirror: x_surface (n_rays,3) = x and depth (n_rays) = |o - x| in place.  mask (n_rays; thresholded) becomes the merged 0/1
 * mask `mask != 0 || hit` in place; mask_bool (n_rays, 1 byte per ray, torch.bool) receives the same, null = skip; *any
 * (int32, device, caller zeroes it, null = skip) is OR-ed with "any merged ray". */
#define MNRF_PLANE_X 0
#define MNRF_PLANE_Y 1
int mnrf_place_mirror(const float* rays, int64_t n_rays, int axis, float position, float normal_x, float normal_y,
                      float normal_z, float rect_u0, float rect_u1, float rect_w0, float rect_w1, float near,
                      float* depth, float* mask, float* normal, float* x_surface, uint8_t* mask_bool, int32_t* any,
                      void* stream);

/* Transform secondary rays (n_rays,8) in place before a reflection-substitution render (eval.py:550-594): with rotation (a
 * HOST array of 9 floats, row-major R; null = none) o = R o and d = l2_normalize(R d) (utils/func.py:5-7); then
 * o = o * scale + (tx, ty, tz).  Columns 6..7 (near, far) are left as they are. */
int mnrf_transform_rays(float* rays, int64_t n_rays, MNRF_HOST const float* rotation, float scale, float tx, float ty, float tz,
                        void* stream);

/* Reflect a newly placed object (eval.py:173-291, app_reflect_newly_placed_objects; the object is a plain NeRF field that
 * the caller renders between these two calls).
 *
 * Move one level's rays (n_rays,8) into the object's frame, OUT OF PLACE (the level's own rays are still needed): with pose
 * (a HOST array of 12 floats, the row-major 3x4 [A | p] of the reference's pose_align; null = none) o = A o + p and
 * d = l2_normalize(A d) (utils/func.py:5-7); then o = o * scale, then o = o + (tx, ty, tz) -- two roundings, as the reference
 * writes them.  Columns 6..7 (near, far) are copied.  out (n_rays,8) must not be rays. */
int mnrf_object_rays(const float* rays, int64_t n_rays, MNRF_HOST const float* pose, float scale, float tx, float ty, float tz,
                     float* out, void* stream);

/* Merge the object's maps into the level's, ordered by depth (eval.py:261-291).  Per ray: d = obj_depth / scale / pose_scale0
 * (two divisions, in that order; pose_scale0 = the norm of the first column of A, 1 without a pose); the object counts where
 * `d > 0 && obj_opacity > 0.8f`, and is hidden by the scene where `d > depth && depth > near` (near = the global
 * hyper-parameter).  Where it counts and is not hidden: rgb (n_rays,3) = obj_rgb, depth (n_rays) = d, mask (n_rays) = 0, in
 * place; every other ray is left as it was.  Comparisons with NaN are false.  mask: null = skip (a level rendered without a
 * mirror head); *n_used (int32, device, caller zeroes it, null = skip) receives the number of rays that took the object. */
int mnrf_object_merge(const float* obj_rgb, const float* obj_depth, const float* obj_opacity, int64_t n_rays, float scale,
                      float pose_scale0, float near, float* rgb, float* depth, float* mask, int32_t* n_used, void* stream);

/* ---- Object bounds: render a placed object only along the rays that can see it.  csrc/mnrf_object_cull.hip.
 *
 * Bounds are a box [box_lo, box_hi] in the OBJECT's frame cut into Rx x Ry x Rz cells; cell (i, j, k) is the closed box
 * lo + (i..i+1, j..j+1, k..k+1) * (hi - lo) / R.  One bit per cell says whether the object may have density there: 32 cells
 * per uint32 along x (cell i is bit i % 32 of word i / 32), rows padded to whole words, so bits holds
 * Rz * Ry * ceil(Rx / 32) words with (k * Ry + j) * ceil(Rx / 32) + i / 32 the word of cell (i, j, k); padding bits are zero. */
#define MNRF_OBJECT_MAX_RES 1024

/* The bits of a density volume.  volume: (Rz+1, Ry+1, Rx+1) float32 samples at the cells' corners (x fastest).  A cell is
 * set when one of its 8 corners has `!(sigma < sigma_min)` (a NaN corner sets the cell); with dilate = 1 the set is then grown
 * by one cell over the 26-neighbourhood (dilate: 0 or 1).  *n_set (int32, device, null = skip) receives the number of set
 * cells.  Deterministic.  Rx, Ry, Rz in 1..MNRF_OBJECT_MAX_RES. */
int mnrf_occupancy_bits(const float* volume, int Rx, int Ry, int Rz, float sigma_min, int dilate, uint32_t* bits,
                        int32_t* n_set, void* stream);

/* Keep the rays of one level (n_rays,8) whose segment can touch a set cell.  pose, scale, tx, ty, tz: as mnrf_object_rays;
 * per ray the object-frame ray q is computed by the very device function of mnrf_object_rays.  box_lo, box_hi: HOST arrays of
 * 3 floats, finite, lo < hi.  bits: null = the whole box counts as one set cell (Rx, Ry, Rz are then not read).
 * The rule, on q as written in fp32, with the segment {o + d z : z in [q[6], q[7]]}:
 *   kept for certain:   a ray whose segment, in exact arithmetic, intersects a set cell; a ray with a non-finite component;
 *   culled for certain: a ray whose segment does not intersect the set cells grown by one cell extent per axis
 * (the implementation decides in float64 against cells grown by 2^-12 of their extent: the band in between is that thin).
 * An empty segment (far < near) is culled.  Kept rays are written compacted and in source order: out_rays (n_rays,8) row p
 * = q of ray index[p], index (n_rays) int32 strictly increasing, *count (int32, device) their number; rows from *count on are
 * not defined (index is also the pass's scratch).  No atomic decides an order.  out_rays must not be rays. */
int mnrf_object_cull(const float* rays, int64_t n_rays, MNRF_HOST const float* pose, float scale, float tx, float ty, float tz,
                     MNRF_HOST const float* box_lo, MNRF_HOST const float* box_hi, int Rx, int Ry, int Rz, const uint32_t* bits,
                     float* out_rays, int32_t* index, int32_t* count, void* stream);

/* mnrf_object_merge's per-ray rule (the same device function) for the kept rays: row i of the object's maps (rendered on
 * out_rays) against row index[i] of the level's maps, for i < min(*count, capacity); *count is read on the device.  Rows of
 * the level's maps that index does not list are not touched.  mask, n_used: as mnrf_object_merge. */
int mnrf_object_merge_indexed(const float* obj_rgb, const float* obj_depth, const float* obj_opacity, const int32_t* index,
                              const int32_t* count, int64_t capacity, float scale, float pose_scale0, float near, float* rgb,
                              float* depth, float* mask, int32_t* n_used, void* stream);

/* ---- Several placed objects at one level: culled in one pass, merged in one pass.  csrc/mnrf_objects.hip.
 *
 * THE RULE, per ray of the level: for k = 0 .. n_objects-1 in list order, the single-object rule of mnrf_object_merge for
 * object k is applied to the ray's CURRENT (rgb, depth, mask) -- current: as left by the scene and by the objects 0 .. k-1.
 * That is, by definition, the chain of n_objects single-object applications.  The rule writes depth = d, so the nearest
 * opaque object wins; an exact tie in depth goes to the LATER object of the list (`d > depth` is false); and a current depth
 * `<= near` hides nothing (eval.py:275-281), whichever object or scene left it. */
#define MNRF_OBJECTS_MAX 8

/* mnrf_object_cull for n_objects (1..MNRF_OBJECTS_MAX) objects on the same rays (n_rays,8), in two launches in all.  Per
 * object, HOST arrays of n_objects rows: posed (0 / 1) and poses (12 floats a row, read where posed), scales, translations
 * (3 a row): the ray move, as mnrf_object_rays; unbounded (0 / 1): 1 = the object has no bounds, every ray is kept and its
 * row is what mnrf_object_rays writes (box_lo, box_hi, res, bits of that object are not read); box_lo, box_hi (3 a row),
 * res (Rx, Ry, Rz a row), bits (a HOST array of n_objects DEVICE pointers, null = the whole box is one set cell): the bounds,
 * as mnrf_object_cull.  Outputs, per object exactly what mnrf_object_cull writes (the same device functions decide):
 * out_rays (n_objects,n_rays,8), index (n_objects,n_rays) int32 -- the kept rays of object k compacted in source order in
 * rows 0 .. counts[k]-1 of plane k, rows from counts[k] on not defined -- counts (n_objects) int32, and slot
 * (n_objects,n_rays) int32: slot[k][r] = the row of ray r in object k's list, or -1.  No atomic decides an order.  rays and
 * out_rays are aligned to 16 bytes and distinct. */
int mnrf_objects_cull(const float* rays, int64_t n_rays, int n_objects, MNRF_HOST const int* posed, MNRF_HOST const float* poses,
                      MNRF_HOST const float* scales, MNRF_HOST const float* translations, MNRF_HOST const int* unbounded,
                      MNRF_HOST const float* box_lo, MNRF_HOST const float* box_hi, MNRF_HOST const int* res,
                      const uint32_t* const* bits, float* out_rays, int32_t* index, int32_t* slot, int32_t* counts, void* stream);

/* THE RULE above on the n_rays rays of a level, in one launch.  obj_rgb, obj_depth, obj_opacity: HOST arrays of n_objects
 * DEVICE pointers, the maps of object k rendered on the rows of its out_rays plane (a null entry, in all three: the object
 * was not rendered and is skipped); slot, counts: of mnrf_objects_cull; row s = slot[k][r] of object k's maps is merged
 * into ray r where 0 <= s < min(counts[k], capacity) (counts is read on the device; a given map of object k holds at
 * least that many rows).  scales, pose_scale0: HOST arrays of n_objects floats; near; rgb, depth, mask: as mnrf_object_merge.
 * n_used (n_objects int32, device, caller zeroes it, null = skip): element k receives the number of rays that took object k
 * when its turn came -- a ray that a later, nearer object takes afterwards counts for both. */
int mnrf_objects_merge(const float* const* obj_rgb, const float* const* obj_depth, const float* const* obj_opacity, int n_objects,
                       const int32_t* slot, const int32_t* counts, int64_t n_rays, int64_t capacity, MNRF_HOST const float* scales,
                       MNRF_HOST const float* pose_scale0, float near, float* rgb, float* depth, float* mask, int32_t* n_used,
                       void* stream);

/* ---- Several new mirrors at one level, on any plane: batched_inference(new_mirrors=[...]).  csrc/mnrf_mirrors.hip.
 *
 * THE RULE, per ray (o, d) of rays (n_rays,8) and the n_mirrors (1..MNRF_MIRRORS_MAX) mirrors in list order.  Every mirror is
 * tested against depth0, the ray's depth as it is BEFORE this call.  All arithmetic is single fp32 operations in the order written.
 * Mirror k gives an intersection x and in-plane coordinates (u, w):
 *   kind MNRF_MIRROR_AXIS  (axes[k], positions[k]; mnrf_place_mirror's very expressions, one shared device function):
 *     t = (position - o_a) / d_a, u = t * d_b + o_b, w = t * d_2 + o_2, x_a = position, x_b = u, x_2 = w;
 *   kind MNRF_MIRROR_FRAME (row k of frames: centre c, in-plane unit axes e_u, e_w; row k of normals: the unit normal n):
 *     e = c - o, num = (n0*e0 + n1*e1) + n2*e2, den = (n0*d0 + n1*d1) + n2*d2, t = num / den, x_j = t * d_j + o_j, r = x - c,
 *     u = (eu0*r0 + eu1*r1) + eu2*r2, w alike with e_w.
 * Row k of rects is (r0, r1, r2, r3), in (u, w).  Shape MNRF_MIRROR_RECT: inside = !(u < r0 || w < r2 || u > r1 || w > r3);
 * MNRF_MIRROR_ELLIPSE, inscribed in the rect: uc = (r0 + r1) * 0.5f, ru = (r1 - r0) * 0.5f, a = (u - uc) / ru, b alike for w,
 * q = a*a + b*b, inside = !(q > 1.f).  A NaN coordinate counts as inside.  Then, as mnrf_place_mirror:
 * dist = sqrtf(e0*e0 + e1*e1 + e2*e2) with e = o - x, s = sum((x - o) * d), blocked = dist > depth0 && depth0 > near,
 * hit = inside && s > 0 && !blocked.  The winner is `best` of
 *     best = -1;  for k = 0 .. n_mirrors-1:  if hit_k && (best < 0 || dist_k <= best_dist) { best = k; best_dist = dist_k; }
 * -- the nearest hit, an exact tie to the LATER mirror, a NaN never replaces a winner.  Only where best >= 0:
 * x_surface (n_rays,3) = x_best, depth (n_rays) = dist_best, normal (n_rays,3) = row best of normals, in place.  Unlike
 * mnrf_place_mirror, the normal of a ray that is inside a mirror's shape but takes no mirror is KEPT.  mask (n_rays;
 * thresholded) becomes `mask != 0 || best >= 0` in place; mask_bool (1 byte per ray, null = skip) receives the same; *any
 * (int32, device, caller zeroes it, null = skip) is OR-ed with "any merged ray"; index (n_rays int32, null = skip) = best.
 * kinds, shapes, axes (read where the kind is AXIS), positions (alike), frames (9 floats a row, read where the kind is FRAME),
 * normals (3 a row), rects (4 a row): HOST arrays of n_mirrors rows; they travel in the kernel's argument block.  One launch. */
#define MNRF_MIRRORS_MAX 8
#define MNRF_MIRROR_AXIS 0
#define MNRF_MIRROR_FRAME 1
#define MNRF_MIRROR_RECT 0
#define MNRF_MIRROR_ELLIPSE 1
int mnrf_place_mirrors(const float* rays, int64_t n_rays, int n_mirrors, MNRF_HOST const int* kinds, MNRF_HOST const int* shapes,
                       MNRF_HOST const int* axes, MNRF_HOST const float* positions, MNRF_HOST const float* frames,
                       MNRF_HOST const float* normals, MNRF_HOST const float* rects, float near, float* depth, float* mask,
                       float* normal, float* x_surface, uint8_t* mask_bool, int32_t* any, int32_t* index, void* stream);

/* THE RULE with the mirror a ray has just left excluded: batched_inference(new_mirrors=, exclude_source_mirror=True).  Every ray
 * of a level carries source (int32): the index in the list of the placed mirror the ray was reflected off at the level DIRECTLY
 * above; -1 for a ray that left the scene's own mirror, for a ray that took no mirror and for a ray of the call itself.  THE
 * RULE changes in one place,
 *     hit_k = inside && s > 0 && !blocked && k != source,
 * and in nothing else: the winner, the ties, the writes, the merged mask, the flag and index are as above.  A source outside
 * 0 .. n_mirrors-1 excludes nothing; the device makes no range check.  Only the mirror left at the level directly above is
 * excluded: a ray may return to it after another bounce.  Why: a ray reflected off a tilted frame mirror starts within an ulp
 * of that mirror's plane, on either side; from behind it, the rule above finds the same mirror again at a distance of 1e-9 to
 * 1e-7, nearer than everything else.
 * source: n_rays int32 on the device, one dword read per ray; null = no ray has one, and the result is mnrf_place_mirrors' bit
 * for bit.  Everything else as mnrf_place_mirrors.  One launch. */
int mnrf_place_mirrors_from(const float* rays, int64_t n_rays, int n_mirrors, MNRF_HOST const int* kinds, MNRF_HOST const int* shapes,
                            MNRF_HOST const int* axes, MNRF_HOST const float* positions, MNRF_HOST const float* frames,
                            MNRF_HOST const float* normals, MNRF_HOST const float* rects, float near, const int32_t* source,
                            float* depth, float* mask, float* normal, float* x_surface, uint8_t* mask_bool, int32_t* any,
                            int32_t* index, void* stream);

/* The source row of the next level: out[j * m + p] = level_index[compaction_index[p]] for j < n_rep, p < m.  level_index: the index
 * mnrf_place_mirrors(_from) wrote at this level, null = this level placed none: -1 everywhere; compaction_index (m) int32: the
 * rays that are reflected, as mnrf_reflect_compact numbers them, null = p itself (level 0 reflects every ray); n_rep >= 1: the
 * jitter blocks of a fan (mnrf_reflect_jitter_fan_rows), each a copy of the first.  Precondition: every compaction_index[p] is a
 * row of level_index (it is a compaction of that level's rays).  out (n_rep * m) int32, distinct from the inputs.  m == 0
 * returns 0 without a launch; a negative m, n_rep < 1 or a null out returns MNRF_ERR_ARG.  One launch. */
int mnrf_mirror_sources(const int32_t* level_index, const int32_t* compaction_index, int64_t m, int n_rep, int32_t* out, void* stream);

/* ---- Mirror roughness on partly mirrored chunks: batched_inference with app_control_mirror_roughness (eval.py:506-511,
 * 622-674).  csrc/mnrf_rough.hip.
 *
 * THE RULE, for a level that traces with roughness on: N rays, the thresholded mask, M = the number of rays with mask != 0,
 * index[p] = the p-th such ray in order (ONE order-preserving compaction per chunk and level -- the one mnrf_reflect_compact
 * with compact = 1 writes -- and one host read of its count, whatever trace_ray_times is).
 *   R, the first secondary render, is as without this rule: at level 0 all N rays are reflected with draw 0 and ray i's row is
 *     i; at levels >= 1 the M mirror rays are reflected and ray index[p]'s row is p.
 *   J_j, j = 1 .. trace_ray_times, is the render of the M compacted reflections of the mirror rays about
 *     l2n(normal + draw_j * std); row p belongs to ray index[p].
 *   A mirror ray, per colour key present (rgb_coarse, rgb_fine): S = ((R[row] + J_1[p]) + J_2[p]) + ..., single fp32 additions
 *     in that order; its reflection colour is S finished by trace_ray_times + 1 (below).
 *   A ray of level 0 that is NOT a mirror ray keeps R[i] unchanged: the mean of the one sample it has (the blend gives it
 *     weight 0 anyway), so rgb_*_reflect stays a consistent image.
 * Where M == N this is the reference's arithmetic (eval.py:661-674); where M < N the reference adds (M,3) to (N,3) tensors,
 * which raises or -- with M == 1 -- broadcasts one ray's colours over the chunk: there is nothing of it to reproduce.
 * Finish: the reference writes `rgb / (trace_ray_times + 1)` (eval.py:671-674); on the device torch evaluates a division by a
 * host scalar as a MULTIPLICATION by the fp32 reciprocal 1.f / (float)(times + 1) (tests/test_hip_rough_kernels.py holds the
 * kernel to torch's own `/`), so the driver passes MNRF_MEAN_MULTIPLY with that reciprocal, formed on the host in fp32. */
#define MNRF_MEAN_NONE 0       /* mnrf_jitter_mean: add only (every group of jitters but the last) */
#define MNRF_MEAN_DIVIDE 1     /* ... then a = a / finish_value (an IEEE fp32 division) */
#define MNRF_MEAN_MULTIPLY 2   /* ... then a = a * finish_value */

/* The n_jit jittered reflections of the m mirror rays of a level in one launch.  rays (n_rays,8), x_surface (n_rays,3), normal
 * (n_rays,3): the level's; noise (n_jit, n_rays, 3): one (n_rays,3) standard-normal draw per jitter, or null (no jitter:
 * every block of sec is the same); index (m) int32: the source rays, each in [0, n_rays) (a row that is not is skipped).
 * Row j * m + p of sec (n_jit * m, 8) = [x_surface_i, r, near2, rays[i][7]] with i = index[p] and r the reflection of ray i about
 * l2n(normal_i + noise[j][i] * noise_std): mnrf_reflect_compact's expressions in its order, so block j equals the sec_rays of
 * mnrf_reflect_compact run with compact = 1 and noise[j].  m == 0 returns 0 without a launch; a null pointer other than noise, a
 * negative size, m > n_rays or n_jit < 1 returns MNRF_ERR_ARG. */
int mnrf_reflect_jitter_fan(const float* rays, const float* x_surface, const float* normal, const float* noise, float noise_std,
                            const int32_t* index, int64_t m, int64_t n_rays, int n_jit, float near2, float* sec, void* stream);

/* The sums of THE RULE, in place on acc (n_acc,3).  pieces (n_jit, m, 3): the colours of n_jit jittered renders; index (m) int32
 * or null.  Per p in [0, m): row = index ? index[p] : p;  a = acc[row];  for j = 0 .. n_jit-1: a = a + pieces[j][p];  then, by
 * finish_mode, nothing, a = a / finish_value or a = a * finish_value;  acc[row] = a.  Rows of acc that index does not name are
 * neither read nor written.  Precondition: the rows of index are distinct (it is a compaction) and lie in [0, n_acc) (a row
 * that does not is skipped); acc and pieces do not overlap.  Calls over consecutive groups of jitters, the last one alone
 * finishing, perform the additions of one call over all of them.  m == 0 returns 0 without a launch. */
int mnrf_jitter_mean(float* acc, const float* pieces, const int32_t* index, int64_t m, int n_jit, int64_t n_acc, int finish_mode,
                     float finish_value, void* stream);

/* ---- A roughness per mirror: batched_inference(rough_times=T, scene_roughness=, new_mirrors=[PlacedMirror(..., roughness=)]).
 * csrc/mnrf_rough.hip.  Not the reference's flag (one std for every mirror ray of the frame, above): the std is a per-ray row.
 *
 * THE RULE, for a level that traces: N rays, the thresholded (and merged) mask, and index (N int32) as mnrf_place_mirrors wrote
 * it at THIS level -- -1 everywhere where no list is placed or the level places none; K mirrors with roughness[k] >= 0.
 *   std_i = roughness[index_i] where 0 <= index_i < K, otherwise scene_roughness (an index outside [-1, K) counts as -1).
 *   The first reflection (every ray at level 0, the mirror rays at levels >= 1) is taken about l2n(normal_i + draw_0[i] * std_i)
 *     where std_i > 0 and about l2n(normal_i), with NO addition, where std_i == 0: the bits of the frame without roughness, a
 *     -0 component included.
 *   J = {i : mask_i != 0 and std_i > 0}.  Each ray of J gets T further reflections about l2n(normal_i + draw_j[i] * std_i),
 *     j = 1 .. T; its reflection colour is ((R + J_1) + J_2) + ... finished as above by T + 1, added through the index of ONE
 *     order-preserving compaction of J per chunk and level.  A mirror ray outside J (a polished mirror) and a ray of level 0
 *     that is no mirror ray keep the single sample they have.
 *   Draws: one (N,3) draw for the first reflection of every tracing level, then T more iff J is not empty at that level -- so
 *     where every std equals S > 0 the draws, the launches' inputs and the result are those of "Mirror roughness" above with
 *     trace_ray_times = T and std S.  Count reads: the mask's (levels >= 1) plus J's per chunk and level, whatever T is. */

/* std_rows (n_rays) = std_i of THE RULE; jitter_mask (n_rays) = 1.f where ray i is in J, else 0.f; *any (int32, device, caller
 * zeroes it, null = skip) is OR-ed with "J is not empty".  index (n_rays int32): null = all -1; mask (n_rays); n_mirrors in
 * 0..MNRF_MIRRORS_MAX; roughness: a HOST array of n_mirrors floats (null allowed where n_mirrors == 0), each finite and >= 0, as
 * scene_roughness; they travel in the kernel's argument block.  n_rays == 0 returns 0 without a launch. */
int mnrf_rough_rows(const int32_t* index, const float* mask, int64_t n_rays, int n_mirrors, MNRF_HOST const float* roughness,
                    float scene_roughness, float* std_rows, float* jitter_mask, int32_t* any, void* stream);

/* out (n_rays,3): per component out_i = std_rows[i] > 0 ? normal_i + noise_i * std_rows[i] : normal_i -- one multiplication and
 * one addition, mnrf_reflect.h's own, or the untouched value.  mnrf_reflect_compact with a null noise pointer on `out` then gives
 * the bits it gives on `normal` with the noise and the std.  normal, noise (n_rays,3); out does not overlap them. */
int mnrf_perturb_normals(const float* normal, const float* noise, const float* std_rows, int64_t n_rays, float* out, void* stream);

/* mnrf_reflect_jitter_fan with the std of source ray i = std_rows[i] (n_rays) in place of noise_std: the same layout (row
 * j * m + p of sec is ray index[p] with draw noise[j][index[p]]), the same expressions (mnrf_reflect.h), the same refusals;
 * std_rows must not be null.  m == 0 returns 0 without a launch; a row whose index is outside [0, n_rays) is not written. */
int mnrf_reflect_jitter_fan_rows(const float* rays, const float* x_surface, const float* normal, const float* noise,
                                 const float* std_rows, const int32_t* index, int64_t m, int64_t n_rays, int n_jit, float near2,
                                 float* sec, void* stream);

/* Backward of mnrf_composite (training). Inputs: the forward inputs (rays, sigma, z_vals, noise,
 * rgb, is_mirror, pred_normal, normal), the forward outputs weights (n_rays,S) and depth (n_rays),
 * and the upstream gradients of every per-ray output (null = zero): g_weights (n_rays,S), g_opacity,
 * g_rgb_map (.,3), g_depth, g_mirror_mask, g_surf_normal (.,3), g_surf_normal_grad (.,3),
 * g_normal_dif, g_x_surface (.,3).
 * Outputs (null = skip): d_sigma (n_rays,S), d_rgb (.,S,3), d_is_mirror (.,S), d_pred_normal (.,S,3),
 * d_normal (.,S,3), d_rays (n_rays,8) [origin and direction gradients through x_surface = o + d*depth].
 * Reference: autograd through models/rendering.py:181-264, 362-367. */
int mnrf_composite_backward(const float* rays, int64_t n_rays, int S, const float* sigma, const float* z_vals,
                            const float* noise, const float* rgb, const float* is_mirror,
                            const float* pred_normal, const float* normal, int white_back,
                            const float* weights, const float* depth,
                            const float* g_weights, const float* g_opacity, const float* g_rgb_map,
                            const float* g_depth, const float* g_mirror_mask, const float* g_surf_normal,
                            const float* g_surf_normal_grad, const float* g_normal_dif, const float* g_x_surface,
                            float* d_sigma, float* d_rgb, float* d_is_mirror, float* d_pred_normal,
                            float* d_normal, float* d_rays,
                            int detach /* MNRF_DETACH_W_* : models/rendering.py:223-247 */,
                            const float* keep_mirror /* (n_rays) or null: 0 = this ray's mirror mask sees weights.detach() */,
                            void* stream);

/* Ray gradients of one field evaluation in ray mode (autograd of models/rendering.py:302 `x = o + d z` and of the per-ray view
 * encoding, rendering.py:275-277): g_rays (n_rays, 8) = [sum_s dL/dx_s | sum_s z_s dL/dx_s | 0 0] from d_xyz (n_rays*spr, 3) and
 * z_vals (n_rays, spr); g_de (n_rays, 27) = sum_s d_dir[s][:27] from d_dir (n_rays*spr, 32).  Either output may be null. */
int mnrf_ray_grads(const float* d_xyz, const float* z_vals, const float* d_dir, int64_t n_rays, int spr, float* g_rays,
                   float* g_de, void* stream);

/* ---- backward of the per-ray glue (training; autograd through train.py:217-296, mirror_nerf.py:20-38)
 * reflect: g_sec (n_sec,8) = dL/d secondary rays -> dL/dx_surface (n_rays,3), dL/d normal (n_rays,3),
 *          dL/d rays (n_rays,8: direction and far columns); rows without a selected ray get zeros.
 * blend:   g_out (n,c) -> dL/d base (n,c) = (1-m) g_out and dL/d sec (n_sec,c) = m g_out gathered by index.
 * embed:   g_out (n, c*(2N+1)) -> dL/dx (n,c). */
int mnrf_reflect_backward(const float* rays, const float* normal, const int32_t* index, int64_t n_sec,
                          const float* g_sec, int64_t n_rays, float* g_x_surface, float* g_normal, float* g_rays,
                          void* stream);
int mnrf_blend_backward(const float* g_out, const float* mask, const int32_t* index, int64_t n_sec, int64_t n, int c,
                        float* g_base, float* g_sec, void* stream);
int mnrf_embed_backward(const float* x, const float* g_out, int64_t n, int c, int n_freqs, float* g_x, void* stream);

/* ---- training (forward with saved activations, backward) -----------------------------------
 * Buffer sizes for B samples: activations (floats), ReLU bit masks (uint64 words), workspace of
 * the backward (floats: pre-activation gradients + split-K partials of the weight gradients). */
int64_t mnrf_train_save_floats(int64_t B);
int64_t mnrf_train_mask_words(int64_t B);
int64_t mnrf_train_workspace_floats(int64_t B);

/* mnrf_field_forward for training: all four heads (+ `normal` when non-null), and keeps in
 * save_x / save_mask / save_inv what mnrf_field_backward needs (no recomputation).  save_x is a workspace without an element
 * type of its own: mnrf_train_save_floats(B) fp32 rows, or with MNRF_TRAIN_PLANES mnrf_train_planes_bytes(B) bytes of f16 tiles. */
int mnrf_field_forward_train(float* packed, int64_t B, const float* xyz, int64_t xyz_stride,
                             const float* rays, const float* z_vals, int spr, const float* dir_emb,
                             int64_t dir_stride, float* sigma, float* rgb, float* pred_normal,
                             float* is_mirror, float* normal, void* save_x, uint64_t* save_mask,
                             float* save_inv, float* save_invj, unsigned flags /* 0 or MNRF_SPLIT_F16 [| MNRF_TRAIN_PLANES] */, void* stream);

/* Backward of the field MLP: given dL/d{sigma (B), rgb (B,3), pred_normal (B,3), is_mirror (B)},
 * writes the gradient of every parameter (d_params: HOST array of MNRF_N_PARAMS device pointers,
 * state_dict order, overwritten), dL/dxyz (B,3) and dL/d(view encoding) (B,32 padded) when non-null.
 * The gradient flowing into `normal` (the normalised density gradient: a second-order term) is
 * handled by mnrf_field_backward2.
 * Autograd equivalent: loss.backward() through models/mirror_nerf.py:101-212. */
int mnrf_field_backward(float* packed, int64_t B, const float* xyz, int64_t xyz_stride,
                        const float* rays, const float* z_vals, int spr,
                        const float* g_sigma, const float* g_rgb, const float* g_pred_normal,
                        const float* g_is_mirror, const float* rgb, const float* pred_normal,
                        const float* is_mirror, const float* save_x, const uint64_t* save_mask,
                        const float* save_inv, float* workspace, float* const* d_params, float* d_xyz,
                        float* d_dir,
                        const float* keep_mirror /* (B/spr) per ray [(B) with xyz] or null: 0 = the mirror head of this ray's
                                                    samples sees geo_feat.detach() (models/mirror_nerf.py:172-183) */,
                        unsigned flags /* MNRF_SPLIT_F16: activation gradients on the f16 pipe; MNRF_CUT_NORMAL_HEAD /
                                          MNRF_CUT_MIRROR_HEAD: that head sees geo_feat.detach() (mirror_nerf.py:157, 169-170);
                                          MNRF_DW_ACCUMULATE: add to d_params */,
                        void* stream);

/* Second-order term of the field backward: the gradient that reaches the trunk weights, sigma.weight
 * and xyz through `normal = l2n(-d sigma/d xyz)` (utils/func.py:10-25 with create_graph=True).
 * g_normal (B,3) = dL/d normal; normal = the forward output; save_invj (B) from the training forward.
 * ADDS to d_params (trunk weights and sigma.weight only) and to d_xyz (when non-null): call it after
 * mnrf_field_backward.  workspace: mnrf_train_workspace2_floats(B) floats. */
int64_t mnrf_train_workspace2_floats(int64_t B);
int mnrf_field_backward2(float* packed, int64_t B, const float* xyz, int64_t xyz_stride,
                         const float* rays, const float* z_vals, int spr, const float* g_normal,
                         const float* normal, const float* save_invj, const uint64_t* save_mask,
                         float* workspace, float* const* d_params, float* d_xyz, unsigned flags /* 0 or MNRF_SPLIT_F16 */, void* stream);

/* The multiresolution hash encoding alone (what tinycudann's Encoding.forward returns, models/mirror_nerf_tcnn.py:225-227), level
 * by level: planes[level * B + sample] = the level's two features (float2), 32 * B floats.  Samples: rows of `xyz` (stride >= 3)
 * or rays + z_vals.  The first of the two launches of mnrf_tcnn_forward(enc_workspace != null); bench.py prices it against the
 * L2 roofline (`hash_grid_variant.gather_roofline`). */
int mnrf_tcnn_encode(const float* table, MNRF_HOST const int64_t* offsets17_host, double log2_per_level_scale, int base_resolution,
                     float bound, int64_t B, const float* xyz, int64_t xyz_stride, const float* rays, const float* z_vals,
                     int spr, float* planes, void* stream);

/* ... with flags (0 or MNRF_TCNN_TABLE_F16), and the half2 copy of a table those launches read (entries = offsets[16]). */
int mnrf_tcnn_encode_flags(const float* table, MNRF_HOST const int64_t* offsets17_host, double log2_per_level_scale, int base_resolution,
                           float bound, int64_t B, const float* xyz, int64_t xyz_stride, const float* rays, const float* z_vals,
                           int spr, float* planes, unsigned flags, void* stream);
int mnrf_tcnn_table_half(const float* table, int64_t entries, void* table_half, void* stream);

/* Measurement aid for the hash-grid field: the rate of independent random gathers of 8 B (a float2 table entry) or 4 B (what
 * an fp16 table would fetch) from a table of `table_bytes` -- the ceiling that bounds that field's kernels once the table is
 * Infinity-Cache resident (bench.py `hash_grid_variant.roofline`).  n_threads (multiple of 256) threads x iters gathers. */
int mnrf_bench_gather(const void* table, int64_t table_bytes, int bytes_per_gather, int64_t n_threads, int iters, float* out,
                      void* stream);

/* ---- ray-fused fine pass (eval, per-ray maps only; round 3) ------------------------------------------------------------
 * mnrf_field_forward (all four heads, split arithmetic) + mnrf_composite in ONE launch for rays of exactly
 * mnrf_fused_samples_per_ray() (= 192 = 64 coarse + 128 importance) samples: a workgroup evaluates one ray, keeps the head
 * outputs in LDS and composites them with the very body of mnrf_composite's kernel -- the maps are identical bit for bit, and
 * no per-sample tensor (36 B per sample written and read back otherwise) touches HBM.  What the reference's eval caller
 * copies to the CPU and nobody reads (eval.py:735-736, SURVEY 3 "result-dict contract") is simply never produced.
 * noise_std = 0 (test_time), no density-gradient normal.  Null map pointers are skipped; weights (n_rays, 192) optional.
 * flags: MNRF_FUSED_WHITE_BACK (the white_back of mnrf_composite; this argument used to be that int, 0 or 1) |
 * MNRF_FUSED_RGB_DEPTH: the caller reads colour and depth only (the last reflection level of a frame, eval.py:676-697) -- the
 * mirror head is not evaluated (the folded stream puts it last and the launch stops in front of it, 1044 instead of 1112 tile
 * pairs per sample) and the compositing forms rgb, depth and opacity alone (weights and x_surface on request); mirror_mask and
 * surf_normal must be null.  The maps it writes equal those of the full launch bit for bit.
 * Returns MNRF_ERR_UNSUPPORTED when the 48-samples-per-wave tuning is off (MNRF_SPLIT48=0). */
#define MNRF_FUSED_WHITE_BACK 1u
#define MNRF_FUSED_RGB_DEPTH 2u
/* MNRF_FUSED_BLENDED_LEVEL: the caller will blend this level's colour with the thresholded mirror mask, m * reflected +
 * (1 - m) * colour with m = 1 where the composited mirror value is not below 0.5 (batched_inference, every level that traces).
 * The colour of such a ray cannot reach the frame, so the launch does not evaluate it: a workgroup is one ray, it runs the
 * mirror head in front of the colour branch, forms the ray's mirror value with the operations of the compositing, and where
 * that is not below 0.5 (a NaN included) it leaves out dir_encoding / view / rgb -- 76 of the 1112 tile pairs -- and writes 0
 * to the ray's rgb_map row.  Every other map, and the rgb_map rows of the rays below 0.5, equal those of the launch without
 * the flag bit for bit.  Needs mirror_mask; not together with MNRF_FUSED_RGB_DEPTH.  (Value 4 stays unused.)  The range guard
 * does not see the colour-branch activations of a ray that is left out: nobody reads them.
 * mnrf_field_composite_fused_pn is the same call with one more output, the per-sample predicted normals (n_rays, 192, 3), or
 * null: with them and `weights` a level can take the ray-fused launch under the full result contract.  A non-null pred_normal
 * or the flag selects the blended-level kernel (which then skips no ray unless the flag is set); pred_normal is refused
 * together with MNRF_FUSED_RGB_DEPTH, whose launch forms no normal. */
#define MNRF_FUSED_BLENDED_LEVEL 8u
int mnrf_fused_samples_per_ray(void);
int mnrf_field_composite_fused(float* packed, int64_t n_rays, const float* rays, const float* z_vals,
                               const float* dir_emb, int64_t dir_stride, int flags,
                               float* weights, float* opacity, float* rgb_map, float* depth, float* mirror_mask,
                               float* surf_normal, float* x_surface, void* stream);
int mnrf_field_composite_fused_pn(float* packed, int64_t n_rays, const float* rays, const float* z_vals,
                                  const float* dir_emb, int64_t dir_stride, int flags,
                                  float* weights, float* opacity, float* rgb_map, float* depth, float* mirror_mask,
                                  float* surf_normal, float* x_surface, float* pred_normal, void* stream);

/* ---- the fp32 -> (hi, lo) conversion of the forward-only split kernels --------------------------------------------------
 * Those kernels form lo = f16(x - hi) with two mixed-precision FMAs under a round-toward-zero f16 mode (8 vector
 * instructions per value pair); the long form (convert, subtract, convert: 11) stays compiled for comparison and gives the
 * same bits.  mnrf_split_convert_long(on): on > 0 puts every later forward-only split launch of this process on the long
 * form, 0 on the short one, a negative value changes nothing; returns the setting it found (initially the environment's
 * MNRF_SPLIT_CONVERT_LONG, read once).  The training kernels always run the long form.
 * mnrf_split2_probe runs the kernels' own conversion, under their mode setting, over n_pairs pairs (x[2i], x[2i+1]) and
 * writes the packed hi and lo words of pair i to hi[i] and lo[i]; relu != 0 passes the values through the kernels' ReLU
 * first, as the in-stream conversion does; long_form != 0 takes the long form. */
int mnrf_split_convert_long(int on);
int mnrf_split2_probe(const float* x, int64_t n_pairs, int relu, int long_form, uint32_t* hi, uint32_t* lo, void* stream);

/* ---- training, round 3: operand planes (split arithmetic only) --------------------------------------------------------
 * The weight gradients dW = dY^T X contract over samples.  With MNRF_TRAIN_PLANES the training forward keeps the inputs X
 * of every Linear -- and mnrf_field_backward_planes the pre-activation gradients dY -- not as fp32 rows but as the hi/lo
 * f16 operand tiles the GEMM consumes directly (layout: mirror_nerf_amd/csrc/mnrf_dwp.h), and ONE call of mnrf_dw_planes
 * computes the gradients of all 32 parameters over ALL evaluations of a module in a backward pass (primary rays, reflected
 * rays ...: train.py:253-259 evaluates the same models at every recursion level).
 * Autograd equivalent: loss.backward() through models/mirror_nerf.py:101-212, .grad accumulated over the evaluations. */
#define MNRF_TRAIN_PLANES 256u     /* mnrf_field_forward_train: `save_x` is a planes buffer of mnrf_train_planes_bytes(B) bytes */
#define MNRF_PLANES_Y_HALF 0x100000u   /* round 6, OPT-IN (flags of mnrf_field_backward_planes; bit 12 = 0x1000 of the evaluation's kinds[e]
                                          entry of mnrf_dw_planes2): dY travels as ONE f16 per element under the planes' per-sample
                                          scale instead of a hi/lo pair -- the producer's lo tiles never reach memory, the GEMM fetches
                                          and multiplies the hi tiles only (3/4 of the GEMM's bytes, half the producer's stores).
                                          NOT exact: 1.2e-4 .. 7.4e-4 of each weight tensor's largest entry against float64 on the
                                          gradient fixtures (profiles/r06_half_planes_emulation.json; bar 1e-3).  Ring GEMM only. */
int64_t mnrf_train_planes_bytes(int64_t B);      /* X planes of B samples (bytes) */
int64_t mnrf_train_dy_planes_bytes(int64_t B);   /* dY planes of B samples (bytes) */

/* Activation gradients only (no weight gradients): mnrf_field_backward's first half on the split arithmetic.  dy_planes
 * (mnrf_train_dy_planes_bytes(B)) receives dY under one power-of-two scale for the whole call, derived from the largest seed
 * magnitude, whose float bits are left in *seedmax (a device word, overwritten) for mnrf_dw_planes.  A null upstream
 * gradient means zero (no tensor of zeros needed for a head no loss reads). */
int mnrf_field_backward_planes(float* packed, int64_t B, const float* xyz, int64_t xyz_stride,
                               const float* rays, const float* z_vals, int spr,
                               const float* g_sigma, const float* g_rgb, const float* g_pred_normal,
                               const float* g_is_mirror, const float* rgb, const float* pred_normal,
                               const float* is_mirror, const uint64_t* save_mask, const float* save_inv,
                               void* dy_planes, uint32_t* seedmax, float* d_xyz, float* d_dir, const float* keep_mirror,
                               unsigned flags /* MNRF_CUT_NORMAL_HEAD | MNRF_CUT_MIRROR_HEAD | r << 16 with r = 0..15: every sample's
                                                 largest seed is scaled to [2^(6-r), 2^(7-r)) instead of [2^6, 2^7) -- 2^r more room
                                                 for gradients that GROW on their way down the trunk (trained weights), r bits
                                                 less for those that shrink; the same r goes to mnrf_dw_planes2 in kinds[e] */,
                               void* stream);

/* Weight gradients of n_eval (1..8) evaluations of one module: x_planes[e] from mnrf_field_forward_train, dy_planes[e] and
 * seedmax[e] from mnrf_field_backward_planes, B[e] their sample counts (HOST arrays).  d_params: HOST array of MNRF_N_PARAMS
 * device pointers, overwritten (accumulate = 0) or added to.  workspace: mnrf_dw_planes_workspace_floats(n_eval, B) floats. */
int64_t mnrf_dw_planes_workspace_floats(int n_eval, MNRF_HOST const int64_t* B);
int mnrf_dw_planes(int n_eval, const void* const* x_planes, const void* const* dy_planes, MNRF_HOST const int64_t* B,
                   const uint32_t* const* seedmax, float* workspace, float* const* d_params, int accumulate, void* stream);

/* Round 4: the second-order term (mnrf_field_backward2) on the planes route.  mnrf_field_backward2_planes runs the tangent pass
 * only and leaves the tangents a' (x2_planes, mnrf_train_planes2_bytes(B)) and the density-gradient signals b (y2_planes,
 * mnrf_train_dy_planes2_bytes(B)) as operand planes under one power-of-two scale for the call, derived from the largest |J^|
 * whose float bits are left in *jmax (a device word, overwritten); ADDS to d_xyz when non-null.  mnrf_dw_planes2 is
 * mnrf_dw_planes with a KIND per evaluation (HOST array, null = all 0; bits 8-11: the r of that evaluation's
 * mnrf_field_backward_planes call): 0 = (x_planes, dy_planes, seedmax) of the first-order
 * calls above, 1 = (x2_planes, y2_planes, jmax) of this one -- the weight gradients of a module over all evaluations and both
 * orders in ONE launch (the reference: one loss.backward() through utils/func.py:10-25 with create_graph=True). */
int64_t mnrf_train_planes2_bytes(int64_t B);
int64_t mnrf_train_dy_planes2_bytes(int64_t B);
int mnrf_field_backward2_planes(float* packed, int64_t B, const float* xyz, int64_t xyz_stride,
                                const float* rays, const float* z_vals, int spr, const float* g_normal,
                                const float* normal, const float* save_invj, const uint64_t* save_mask,
                                void* x2_planes, void* y2_planes, uint32_t* jmax, float* d_xyz, void* stream);
int64_t mnrf_dw_planes2_workspace_floats(int n_eval, MNRF_HOST const int64_t* B, MNRF_HOST const int* kinds);
int mnrf_dw_planes2(int n_eval, const void* const* x_planes, const void* const* dy_planes, MNRF_HOST const int64_t* B,
                    const uint32_t* const* seedmax, MNRF_HOST const int* kinds, float* workspace, float* const* d_params, int accumulate,
                    void* stream);

/* ---- optimizer step (training.FlatAdam) ------------------------------------------------------------------------------------
 * Adam over ONE flat tensor of n floats (16-byte aligned; a field model's 595 k parameters as views of one buffer, its gradient
 * the flat buffer the backward pass produced): torch.optim.Adam's update (non-amsgrad, L2 weight decay; utils/__init__.py
 * get_optimizer builds that optimizer, train.py:101-109) with one thread per four elements -- torch's fused multi-tensor kernel
 * gives such a tensor ten thread blocks.  `step` = the caller's count of calls (this one included), `*skipped` (device, the
 * caller zeroes it once) = how many of them found_inf has voided: with *found_inf != 0 nothing is updated and *skipped grows by
 * one, as torch's fused Adam does under GradScaler; grad_scale / found_inf may be null.  The bias corrections (for step -
 * *skipped, at least 1) and 1 - beta1, 1 - beta2 are formed in double and rounded to float once; per element the arithmetic is
 * float, both moments updated as x + (1 - beta)(new - x). */
int mnrf_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, double beta1,
                   double beta2, float eps, float weight_decay, int64_t step, int32_t* skipped, const float* grad_scale,
                   const float* found_inf, void* stream);

/* ---- live row counts on the device (round 5): a training step without a host round trip -------------------------------------
 * Training traces the reflections of exactly the rays the mirror mask selects (train.py:170-178, 248-252).  How many those are
 * is known on the device only (*count of mnrf_reflect_compact); the reference reads it on the host (`mask.any()`, then boolean
 * indexing: one stream sync in the middle of every step).  Every `_n` entry point below is its namesake with ONE more argument
 * in front of `stream`: `n_live`, a DEVICE int32 holding the number of rows (rays; samples / spr for the field entry points)
 * that exist.  The row-count argument becomes the CAPACITY the buffers are sized for: the launch is sized for it, workgroups
 * past the live rows leave at once, rows past them are neither read nor written.  n_live == null: exactly the namesake.  The
 * field entry points at the end of this section (mnrf_field_forward_train_n, mnrf_field_backward_planes_n,
 * mnrf_field_backward2_planes_n, mnrf_dw_planes2_n) clamp a count outside [0, capacity]: below zero nothing exists, above the
 * capacity every row does.  They work in whole 128-sample tiles: the mask words and operand planes of the first
 * ceil(*n_live * spr / 128) tiles are written (what the namesake writes for that many samples), nothing past them; with nothing
 * live no output is written, an overwriting mnrf_dw_planes2_n leaves zeros and an accumulating one changes nothing.  With
 * them the forward, backward and optimizer launches of a whole step are a fixed sequence -- capturable as ONE hipGraph
 * (mirror_nerf_amd.training.GraphedTrainStep).  Field entry points: MNRF_SPLIT_F16 | MNRF_TRAIN_PLANES route only. */
int mnrf_embed_n(const float* x, int64_t n, int c, int n_freqs, float* out, const int32_t* n_live, void* stream);
int mnrf_embed_backward_n(const float* x, const float* g_out, int64_t n, int c, int n_freqs, float* g_x, const int32_t* n_live, void* stream);
int mnrf_sample_coarse_n(const float* rays, int64_t n_rays, const float* z_steps, int n_samples, int use_disp, float perturb,
                         const float* perturb_rand, float* z_vals, const int32_t* n_live, void* stream);
/* What render_rays does with a ray before the first field evaluation (models/rendering.py:275-300: `embedding_dir(rays_d)`, the
 * coarse depths) as one launch: dir_emb (n_rays, 3 (2 n_freqs_dir + 1)) = mnrf_embed of columns 3..5 of the rays read in place,
 * z_vals = mnrf_sample_coarse; both bit for bit.  n_samples >= 3. */
int mnrf_ray_prologue_n(const float* rays, int64_t n_rays, int n_freqs_dir, const float* z_steps, int n_samples, int use_disp,
                        float perturb, const float* perturb_rand, float* dir_emb, float* z_vals, const int32_t* n_live, void* stream);
/* The gradient of reflected rays that went into several consumers (train.py:205: the reflected rays carry gradient back to the
 * surface) in one launch instead of autograd's pairwise adds:
 * g_rays = ((((g0 + g1) + g2) + g3) + pad(mnrf_embed_backward(rays[:, 3:6], g_dir_a + g_dir_b))), sums in this order; g0..g3
 * (n_rays, 8) and g_dir_a / g_dir_b (n_rays, 3 (2 n_freqs_dir + 1)) may each be null (at least one is not). */
int mnrf_ray_fan_backward_n(const float* g0, const float* g1, const float* g2, const float* g3, const float* rays,
                            const float* g_dir_a, const float* g_dir_b, int64_t n_rays, int n_freqs_dir, float* g_rays,
                            const int32_t* n_live, void* stream);
int mnrf_composite_n(const float* rays, int64_t n_rays, int S, const float* sigma, const float* z_vals,
                     const float* noise, const float* rgb, const float* is_mirror,
                     const float* pred_normal, const float* normal, int white_back,
                     float* weights, float* opacity, float* rgb_map, float* depth, float* mirror_mask,
                     float* surf_normal, float* surf_normal_grad, float* normal_dif, float* x_surface,
                     const int32_t* n_live, void* stream);
/* mnrf_composite_n and the mnrf_sample_fine_n that follows it in a coarse pass (models/rendering.py:181-264, then 312-326) as one
 * launch: z_fine (n_rays, S + n_importance) from these weights; u / u_per_ray / n_importance as in mnrf_sample_fine.  weights must
 * not be null.  Same maps, weights and depths bit for bit. */
int mnrf_composite_sample_n(const float* rays, int64_t n_rays, int S, const float* sigma, const float* z_vals,
                            const float* noise, const float* rgb, const float* is_mirror,
                            const float* pred_normal, const float* normal, int white_back,
                            float* weights, float* opacity, float* rgb_map, float* depth, float* mirror_mask,
                            float* surf_normal, float* surf_normal_grad, float* normal_dif, float* x_surface,
                            const float* u, int u_per_ray, int n_importance, float* z_fine,
                            const int32_t* n_live, void* stream);
int mnrf_composite_backward_n(const float* rays, int64_t n_rays, int S, const float* sigma, const float* z_vals,
                              const float* noise, const float* rgb, const float* is_mirror,
                              const float* pred_normal, const float* normal, int white_back,
                              const float* weights, const float* depth,
                              const float* g_weights, const float* g_opacity, const float* g_rgb_map,
                              const float* g_depth, const float* g_mirror_mask, const float* g_surf_normal,
                              const float* g_surf_normal_grad, const float* g_normal_dif, const float* g_x_surface,
                              float* d_sigma, float* d_rgb, float* d_is_mirror, float* d_pred_normal,
                              float* d_normal, float* d_rays, int detach, const float* keep_mirror,
                              const int32_t* n_live, void* stream);
int mnrf_sample_fine_n(const float* z_coarse, const float* weights, int64_t n_rays, int S,
                       const float* u, int u_per_ray, int n_importance, float* z_fine, const int32_t* n_live, void* stream);
int mnrf_threshold_mask_n(float* mask, int64_t n, int32_t* any, const int32_t* n_live, void* stream);
/* n_live: the live rows of the INPUT rays (a second bounce: the first bounce's count); *count as in the namesake */
int mnrf_reflect_compact_n(const float* rays, const float* x_surface, const float* normal,
                           const float* normal_noise, float noise_std, const float* mask,
                           int64_t n_rays, int compact, float near2, float* sec_rays, int32_t* index,
                           int32_t* count, float* reflect_dir, const int32_t* n_live,
                           int32_t* slot /* (n_rays) or null: the inverse of `index` -- the row of sec_rays ray i went to, -1 where it
                                            was not selected: what the gather-form blend below reads */,
                           void* stream);
/* mnrf_reflect_backward in gather form through `slot` (the static route): every live ray's row of the three outputs is written -- zeros
 * where the ray was not reflected -- so nothing is zero-filled in front; same values.  n_live: the live rows of the INPUT rays. */
int mnrf_reflect_backward_gather_n(const float* rays, const float* normal, const int32_t* slot, const float* g_sec, int64_t n_rays,
                                   float* g_x_surface, float* g_normal, float* g_rays, const int32_t* n_live, void* stream);
/* Both blends of a recursion level (rgb_coarse and rgb_fine, train.py:263-296) in one launch, gather form through `slot`:
 * out = m * part + (1 - m) * base, part = sec[slot[i]] where ray i was reflected and base[i] where not -- mnrf_blend_scatter's
 * expressions, bit-identical values.  Tensor b (or a) may be null.  Backward: g_base = (1 - m) g_out for every live row, g_sec[slot[i]]
 * = m g_out where slot[i] >= 0 (rows of g_sec past the reflection's count are not written). */
int mnrf_blend2_n(const float* base_a, const float* sec_a, const float* base_b, const float* sec_b, const int32_t* slot,
                  const float* mask, int64_t n, int c, float* out_a, float* out_b, const int32_t* n_live, void* stream);
int mnrf_blend2_backward_n(const float* g_out_a, const float* g_out_b, const int32_t* slot, const float* mask, int64_t n, int c,
                           float* g_base_a, float* g_sec_a, float* g_base_b, float* g_sec_b, const int32_t* n_live, void* stream);
/* n_sec_live: live rows of sec / index / g_sec (the reflection's count); n_live: live rows of base / mask / out */
int mnrf_blend_scatter_n(const float* base, const float* sec, const int32_t* index, int64_t n_sec,
                         const float* mask, int64_t n, int c, float* out, float* reflect_out,
                         const int32_t* n_sec_live, const int32_t* n_live, void* stream);
int mnrf_reflect_backward_n(const float* rays, const float* normal, const int32_t* index, int64_t n_sec,
                            const float* g_sec, int64_t n_rays, float* g_x_surface, float* g_normal, float* g_rays,
                            const int32_t* n_sec_live, void* stream);
int mnrf_blend_backward_n(const float* g_out, const float* mask, const int32_t* index, int64_t n_sec, int64_t n, int c,
                          float* g_base, float* g_sec, const int32_t* n_sec_live, const int32_t* n_live, void* stream);
int mnrf_ray_grads_n(const float* d_xyz, const float* z_vals, const float* d_dir, int64_t n_rays, int spr, float* g_rays,
                     float* g_de, const int32_t* n_live, void* stream);
int mnrf_field_forward_train_n(float* packed, int64_t B, const float* xyz, int64_t xyz_stride,
                               const float* rays, const float* z_vals, int spr, const float* dir_emb,
                               int64_t dir_stride, float* sigma, float* rgb, float* pred_normal,
                               float* is_mirror, float* normal, void* save_x, uint64_t* save_mask,
                               float* save_inv, float* save_invj, unsigned flags, const int32_t* n_live, void* stream);
int mnrf_field_backward_planes_n(float* packed, int64_t B, const float* xyz, int64_t xyz_stride,
                                 const float* rays, const float* z_vals, int spr,
                                 const float* g_sigma, const float* g_rgb, const float* g_pred_normal,
                                 const float* g_is_mirror, const float* rgb, const float* pred_normal,
                                 const float* is_mirror, const uint64_t* save_mask, const float* save_inv,
                                 void* dy_planes, uint32_t* seedmax, float* d_xyz, float* d_dir, const float* keep_mirror,
                                 unsigned flags, const int32_t* n_live, void* stream);
int mnrf_field_backward2_planes_n(float* packed, int64_t B, const float* xyz, int64_t xyz_stride,
                                  const float* rays, const float* z_vals, int spr, const float* g_normal,
                                  const float* normal, const float* save_invj, const uint64_t* save_mask,
                                  void* x2_planes, void* y2_planes, uint32_t* jmax, float* d_xyz,
                                  const int32_t* n_live, void* stream);
/* mnrf_dw_planes2 with the sample count of evaluation e on the device: *n_live[e] * spr[e] samples (n_live[e] null: B[e]); B[e]
 * = the capacity its planes were sized for.  n_live, spr: HOST arrays of n_eval entries.  The work plan of the GEMM (which
 * workgroup contracts which 32-sample stages) is made by a one-workgroup launch in front of it and lives at the head of the
 * workspace: mnrf_dw_planes2_n_workspace_floats(n_eval) floats, whatever the counts. */
int64_t mnrf_dw_planes2_n_workspace_floats(int n_eval);
int mnrf_dw_planes2_n(int n_eval, const void* const* x_planes, const void* const* dy_planes, MNRF_HOST const int64_t* B,
                      const int32_t* const* n_live, MNRF_HOST const int* spr, const uint32_t* const* seedmax, MNRF_HOST const int* kinds,
                      float* workspace, float* const* d_params, int accumulate, void* stream);
/* mnrf_adam_step with every scalar of the step in DEVICE memory (a captured step must not freeze the learning rate or the step
 * count).  mnrf_adam_prep, one thread: *step += 1 (the count of steps, this one included, vetoed ones too), then
 * state[0..MNRF_ADAM_STATE_FLOATS) = [veto, lr / bias correction 1, sqrt(bias correction 2), 1 - beta1, 1 - beta2,
 * 1 / grad_scale, eps, weight_decay] from hyper = [lr, beta1, beta2, eps, weight_decay] (doubles; lr, eps and weight_decay are
 * rounded to float as mnrf_adam_step's arguments are; the bias corrections and 1 - beta are formed in double and rounded once,
 * as mnrf_adam_step forms them: the update uses no beta in float) and *skipped (the first model's counter of vetoed steps; the
 * step the corrections are made for is *step - *skipped, at least 1); veto = *found_inf != 0 or any of the 0..4 range-guard
 * words (HOST array of device words: the last word of a packed image) non-zero.  mnrf_adam_step_dev: the update of one flat
 * tensor from `state`, bit for bit mnrf_adam_step's given the same scalars. */
#define MNRF_ADAM_STATE_FLOATS 8
int mnrf_adam_prep(const double* hyper, int64_t* step, const int32_t* skipped, const float* grad_scale, const float* found_inf,
                   const uint32_t* const* guard_words, int n_guard_words, float* state, void* stream);
int mnrf_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* state,
                       int32_t* skipped, void* stream);
/* mnrf_adam_step_dev for up to 4 flat tensors in ONE launch (a step's coarse and fine model): arrays of n_tensors entries each. */
int mnrf_adam_step_dev_n(int n_tensors, float* const* param, const float* const* grad, float* const* exp_avg, float* const* exp_avg_sq,
                         MNRF_HOST const int64_t* n, const float* state, int32_t* const* skipped, void* stream);

/* ---- SGD with momentum and RAdam over one flat fp32 tensor (training.FlatSGD, training.FlatRAdam; utils/__init__.py:47-74
 * get_optimizer's other two torch optimizers), in mnrf_adam_step's shape and under its contract: one thread per four elements,
 * 16-byte aligned tensors, `step` = the caller's count of calls (this one included), `*skipped` (device, zeroed once by the
 * caller) = how many of them were vetoed; with *found_inf != 0 nothing is updated and *skipped grows by one; grad_scale /
 * found_inf may be null.  Each has a device-state form as Adam has: `*_prep`, one thread: *step += 1 (vetoed steps too), then
 * the scalars of the step -> state[]; veto = *found_inf != 0 or any of the 0..4 range-guard words (HOST array of device words)
 * non-zero; `*_step_dev_n`: the update of 0..4 flat tensors from `state` in ONE launch (arrays of n_tensors entries), bit for
 * bit the host-scalar entry point's given the same scalars.
 *
 * SGD is torch.optim.SGD with dampening 0, no Nesterov, L2 weight decay:
 *     G = g / grad_scale + weight_decay p,   buf' = momentum buf + G,   p' = p - lr buf'
 * all in float: G with one rounding per operation (g * (1.f / grad_scale) for the quotient, skipped where grad_scale is null or
 * 1), buf' = fmaf(momentum, buf, G) and p' = fmaf(-lr, buf', p) with one rounding each, as torch's fused SGD computes them; a
 * zero-initialised buffer makes the first step torch's buf = G.  Nothing depends on the step: `step` is checked (>= 1) only.
 * mnrf_sgd_prep: hyper = [lr, momentum, weight_decay] (doubles, rounded to float as mnrf_sgd_step's arguments are);
 * state[0..MNRF_SGD_STATE_FLOATS) = [veto, lr, momentum, 1 / grad_scale, weight_decay]. */
#define MNRF_SGD_STATE_FLOATS 5
int mnrf_sgd_step(float* param, const float* grad, float* momentum_buffer, int64_t n, float lr, float momentum, float weight_decay,
                  int64_t step, int32_t* skipped, const float* grad_scale, const float* found_inf, void* stream);
int mnrf_sgd_prep(const double* hyper, int64_t* step, const int32_t* skipped, const float* grad_scale, const float* found_inf,
                  const uint32_t* const* guard_words, int n_guard_words, float* state, void* stream);
int mnrf_sgd_step_dev_n(int n_tensors, float* const* param, const float* const* grad, float* const* momentum_buffer,
                        MNRF_HOST const int64_t* n, const float* state, int32_t* const* skipped, void* stream);
/* RAdam is torch.optim.RAdam with decoupled_weight_decay=False.  For the effective step t = step - *skipped, at least 1:
 *     G = g / grad_scale + weight_decay p,   m' = m + (1 - beta1)(G - m),   v' = v + (1 - beta2)(G^2 - v)
 *     rho_inf = 2 / (1 - beta2) - 1,   rho_t = rho_inf - 2 t beta2^t / (1 - beta2^t)
 *     rho_t > 5:   p' = p - lr / (1 - beta1^t) * sqrt(1 - beta2^t) r_t * m' / (sqrt(v') + eps)
 *                  r_t = sqrt((rho_t - 4)(rho_t - 2) rho_inf / ((rho_inf - 4)(rho_inf - 2) rho_t))
 *     otherwise:   p' = p - lr / (1 - beta1^t) * m'
 * 1 - beta1^t, the product sqrt(1 - beta2^t) r_t, 1 - beta1 and 1 - beta2 are formed in double from the double betas and
 * rounded to float once; lr (a float) is divided by the rounded 1 - beta1^t in float, as mnrf_adam_step's is; rho_t > 5 is
 * decided in double where the scalars are formed -- in mnrf_radam_prep from the DEVICE count, so a captured step passes from the
 * unrectified to the rectified steps by itself.  Per element the arithmetic is float, one rounding per operation, no beta in
 * float: a = (lr / bc1) * (sqrt(bc2) r_t), p' = p - a * (m' / (sqrtf(v') + eps)), or p' = p - (lr / bc1) * m'.
 * mnrf_radam_prep: hyper = [lr, beta1, beta2, eps, weight_decay] (mnrf_adam_prep's block); state[0..MNRF_RADAM_STATE_FLOATS) =
 * [veto, lr / (1 - beta1^t), sqrt(1 - beta2^t) r_t (0 where not rectified), 1 - beta1, 1 - beta2, 1 / grad_scale, eps,
 * weight_decay, rectified (1 or 0)]. */
#define MNRF_RADAM_STATE_FLOATS 9
int mnrf_radam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, double beta1,
                    double beta2, float eps, float weight_decay, int64_t step, int32_t* skipped, const float* grad_scale,
                    const float* found_inf, void* stream);
int mnrf_radam_prep(const double* hyper, int64_t* step, const int32_t* skipped, const float* grad_scale, const float* found_inf,
                    const uint32_t* const* guard_words, int n_guard_words, float* state, void* stream);
int mnrf_radam_step_dev_n(int n_tensors, float* const* param, const float* const* grad, float* const* exp_avg,
                          float* const* exp_avg_sq, MNRF_HOST const int64_t* n, const float* state, int32_t* const* skipped,
                          void* stream);

/* ---- hash-grid field, BASELINE config 5 (models/mirror_nerf_tcnn.py:151-259) ---------------------
 * table: (entries, 2) fp32 hash-grid features; offsets17_host: 17 level offsets in entries (HOST);
 * log2_per_level_scale, base_resolution, bound: the encoding configuration (mirror_nerf_tcnn.py:36-49);
 * weights: mnrf_tcnn_weight_floats() floats = [sigma_net.0 (64x32) | sigma_net.1 (16x64) | color_net.0
 * (64x32, col 31 zero) | color_net.1 (64x64) | color_net.2 (3x64) | normal_net.0 (64x16, col 15 zero) |
 * normal_net.1 (3x64) | is_mirror_net.0 (32x16, col 15 zero) | its bias (32) | is_mirror_net.2 (1x32) |
 * its bias (1)], rows padded to a multiple of 4.
 * Positions/directions: `xyz` rows [x y z dx dy dz] (stride >= 6, or >= 3 with SIGMA_ONLY), or rays+z_vals
 * with per-ray raw directions `dirs` (null: the ray direction).  sigma is the RAW output h[0] (the ReLU is
 * applied at compositing, mirror_nerf_tcnn.py:235).  geo_feat: (B,15).  Parity vs tinycudann: unpinned. */
int mnrf_tcnn_weight_floats(void);
/* The blob from the model's 11 MLP parameter tensors (HOST array of device pointers in the order above: contiguous fp32 in
 * nn.Linear layout, models/mirror_nerf_tcnn.py:51-149) in one launch; padded columns and the tail are written as zeros. */
int mnrf_tcnn_pack_weights(const float* const* params, float* weights, void* stream);
int mnrf_tcnn_forward(const float* table, MNRF_HOST const int64_t* offsets17_host, double log2_per_level_scale,
                      int base_resolution, float bound, const float* weights, unsigned flags, int64_t B,
                      const float* xyz, int64_t xyz_stride, const float* rays, const float* z_vals, int spr,
                      const float* dirs, int64_t dir_stride, float* sigma, float* rgb, float* pred_normal,
                      float* is_mirror, float* normal, float* geo_feat, float* enc_workspace, void* stream);
/* enc_workspace: null, or 32 * B floats of the caller's memory.  With it the full / f16 evaluations on the matrix pipe run as
 * TWO launches: a level-major encoding pass (grid y = level: the whole device gathers from one 4 MB level at a time, so the
 * XCDs' L2s hold it) that writes the 16 x float2 encoding of every sample into the workspace, and the MLP kernel reading it.
 * Without it every wave walks all 16 levels itself (one launch; 3.2x the table bytes over the fabric at 32768-ray chunks). */

/* Backward of mnrf_tcnn_forward (training of config 5: autograd through mirror_nerf_tcnn.py:220-259,
 * gridencoder.cu:275-380 kernel_grid_backward, shencoder.cu:81-160).  Same inputs as the forward (full evaluation);
 * g_*: dL/d(sigma (B), rgb (B,3), pred_normal (B,3), is_mirror (B)), any may be null (= zero).  ACCUMULATES into
 * d_table (entries,2) and d_weights (mnrf_tcnn_weight_floats() floats, the layout of `weights`; padded columns
 * receive zeros): the caller zero-initialises both, and `workspace` (mnrf_tcnn_backward_workspace_floats() floats:
 * private per-XCD copies of the coarse levels' gradient, folded into d_table at the end; null = none).  Optional outputs d_xyz (B,3) = dL/d position, d_dir (B,3) =
 * dL/d raw direction.  Nothing is saved by the forward: the kernel re-evaluates each tile.
 * g_normal (B,3) or null: dL/d(`normal` of the forward, the normalised density gradient).  When given, a second kernel
 * adds the SECOND-ORDER term -- the gradient that reaches the table, sigma_net and the position through
 * normal = l2n(-d sigma/dx), i.e. what autograd.grad(sigma, x, create_graph=True) propagates in
 * models/mirror_nerf_tcnn.py:172-218 / utils/func.py:10-25 -- to d_table, d_weights and d_xyz. */
int64_t mnrf_tcnn_backward_workspace_floats(MNRF_HOST const int64_t* offsets17_host);
int64_t mnrf_tcnn_backward_workspace_floats2(MNRF_HOST const int64_t* offsets17_host, unsigned flags /* MNRF_TCNN_GRAD_F16 or 0 */);
/* With MNRF_TCNN_GRAD_F16 the LAST FOUR floats of that workspace are an overflow word (uint32, first of the four): non-zero after
 * the call when a half2 sum left the f16 range (it was clamped to +-65504 / scale, not inf) -- fall back to fp32 atomics then. */
int64_t mnrf_tcnn_backward_workspace_floats3(MNRF_HOST const int64_t* offsets17_host, unsigned flags, int64_t B);
int mnrf_tcnn_backward(const float* table, MNRF_HOST const int64_t* offsets17_host, double log2_per_level_scale,
                       int base_resolution, float bound, const float* weights, int64_t B, const float* xyz,
                       int64_t xyz_stride, const float* rays, const float* z_vals, int spr, const float* dirs,
                       int64_t dir_stride, const float* g_sigma, const float* g_rgb, const float* g_pred_normal,
                       const float* g_is_mirror, const float* g_normal, float* workspace, float* d_table,
                       float* d_weights, float* d_xyz, float* d_dir,
                       const float* keep_mirror /* (B/spr) per ray [(B) with xyz] or null: 0 = the mirror head of this ray's samples
                                                   sees geo_feat.detach() (models/mirror_nerf_tcnn.py:200-215) */,
                       unsigned flags /* MNRF_CUT_NORMAL_HEAD / MNRF_CUT_MIRROR_HEAD: that head sees geo_feat.detach()
                                         (mirror_nerf_tcnn.py:186-190, 196-199); MNRF_TCNN_GRAD_F16: see there */,
                       void* stream);

/* Round 6 -- live row counts for the hash-grid field (config 5 on the static training route, see "live row counts on the device"
 * below): ray mode only; B = the capacity the buffers (and the [level][B] planes) are sized for, the kernels evaluate / differentiate
 * the first *n_live * spr samples; rows past them are neither read nor written and add nothing to any gradient.  n_live null =
 * mnrf_tcnn_forward / mnrf_tcnn_backward. */
int mnrf_tcnn_forward_n(const float* table, MNRF_HOST const int64_t* offsets17_host, double log2_per_level_scale,
                        int base_resolution, float bound, const float* weights, unsigned flags, int64_t B,
                        const float* xyz, int64_t xyz_stride, const float* rays, const float* z_vals, int spr,
                        const float* dirs, int64_t dir_stride, float* sigma, float* rgb, float* pred_normal,
                        float* is_mirror, float* normal, float* geo_feat, float* enc_workspace, const int32_t* n_live, void* stream);
int mnrf_tcnn_backward_n(const float* table, MNRF_HOST const int64_t* offsets17_host, double log2_per_level_scale,
                         int base_resolution, float bound, const float* weights, int64_t B, const float* xyz,
                         int64_t xyz_stride, const float* rays, const float* z_vals, int spr, const float* dirs,
                         int64_t dir_stride, const float* g_sigma, const float* g_rgb, const float* g_pred_normal,
                         const float* g_is_mirror, const float* g_normal, float* workspace, float* d_table,
                         float* d_weights, float* d_xyz, float* d_dir, const float* keep_mirror, unsigned flags,
                         const int32_t* n_live, void* stream);

/* Pin-hole ray generation on device (datasets/ray_utils.py:6-53): rays (H*W, 8). */
int mnrf_generate_rays(int H, int W, float focal, MNRF_HOST const float* c2w_host12, float near, float far,
                       float* rays, void* stream);

/* ---- loss reductions of the training step (losses.py:7-255: ColorLoss, MirrorMaskLoss, PlaneConsistentLoss,
 * NormalLoss, NormalRegLoss, TotalLoss), value and gradient in one pass.  Index [0] = coarse, [1] = fine; a null
 * input pointer = "key absent from the result dict" (losses.py tests `f"rgb_{typ}" in inputs`).  Every g_* buffer
 * receives d(total)/d(input) (same shape as the input; may be null).  `out` (6 floats): color, mirror_mask, plane,
 * normal, normal_reg (each already multiplied by its coefficient; 0 when the term is switched off), total.
 * In the train_geometry_stage / invalid-GT branch of ColorLoss the reference thresholds the predicted mask IN PLACE
 * (losses.py:27-33, a detach() shares storage); so does this entry point: mirror_mask[] is not const. */
#define MNRF_LOSS_GEOMETRY_STAGE 1u              /* train_geometry_stage */
#define MNRF_LOSS_WO_MASK_RGB_TO_BLACK 2u        /* hparams.woMaskRGBtoBlack */
#define MNRF_LOSS_NORMAL_ONLY_INSIDE_MIRROR 4u   /* hparams.normal_loss_only_inside_mirror */
#define MNRF_LOSS_EXT_GRAD_NORMAL 8u             /* NormalRegLoss.ext_supervise_grad_normal (default on) */
#define MNRF_LOSS_TCNN_BCE 16u                   /* model_type == "nerf_tcnn": utils/func.py:32-37 instead of nn.BCELoss */
#define MNRF_LOSS_USE_MASK 32u                   /* epoch gates of TotalLoss.forward (losses.py:233-249) */
#define MNRF_LOSS_USE_PLANE 64u
#define MNRF_LOSS_USE_NORMAL 128u
#define MNRF_LOSS_PLANE_ON_DEVICE 256u           /* PlaneConsistentLoss with no host read (round 6): the quadruples are drawn by the
                                                    kernel as floor(plane_u * M) from M = the number of GT-mirror rows the count launch
                                                    of the same call leaves in the workspace; M // 4 of the plane_cap quadruples are
                                                    live (none when a GT entry is invalid, losses.py:116-119); plane_idx / plane_times
                                                    are not read */
typedef struct {
    const float* rgb[2];          /* (N,3) */
    float* mirror_mask[2];        /* (N)   */
    const float* normal_dif[2];   /* (N)   */
    const float* pred_normal[2];  /* (N,S,3) */
    const float* weights[2];      /* (N,S) */
    const float* x_surface[2];    /* (N,3) */
    const float* normal_fine;     /* (N,S_fine,3) */
    int n_samples[2];
    const float* targets;         /* batch["rgbs"] (N,3) */
    const float* gt_mask;         /* batch["mirror_mask"] (N) as float, < 0 = invalid; null = absent */
    const float* rays;            /* batch["rays"] (N,8): directions in columns 3..5 */
    const unsigned char* valid_mask;   /* batch["valid_mask"] (N) or null */
    int64_t n_rays;
    const int64_t* plane_idx[2];  /* (times,4) draws of torch.randint, rows of the GT-mirror subset */
    int64_t plane_times[2];
    const float* plane_u[2];      /* MNRF_LOSS_PLANE_ON_DEVICE: (plane_cap,4) uniform numbers in [0,1); plane_cap >= n_rays / 4 */
    int64_t plane_cap[2];
    float w_color, w_normal, w_normal_reg, w_mask, w_plane;
    unsigned flags;
    float* g_rgb[2];
    float* g_mirror_mask[2];
    float* g_normal_dif[2];
    float* g_pred_normal[2];
    float* g_weights[2];
    float* g_x_surface[2];
    float* g_normal_fine;
    float* out;
} MnrfLossArgs;
int64_t mnrf_loss_workspace_floats(int64_t n_rays, int n_samples_coarse, int n_samples_fine, int64_t plane_times);
int mnrf_total_loss(const MnrfLossArgs* args, float* workspace, void* stream);
/* counts only: workspace[0] = #rays with gt < 0, workspace[1] = #rays with gt != 0 (what the plane loss draws from) */
int mnrf_loss_count(const MnrfLossArgs* args, float* workspace, void* stream);

/* metrics.py:5-15 on device: out[0] = mse = mean((pred - gt)^2) over the n elements whose mask byte is non-zero
 * (mask may be null; element i uses mask[i / per_mask], so per_mask = 3 selects whole RGB pixels), out[1] = psnr =
 * -10 log10(mse), out[2] = number of elements.  `partials`: 2 * mnrf_mse_blocks() floats.  Deterministic. */
int mnrf_mse_blocks(void);
int mnrf_mse_psnr(const float* pred, const float* gt, const unsigned char* mask, int64_t n, int per_mask,
                  float* partials, float* out, void* stream);

/* Structural similarity on the device (csrc/mnrf_metrics.hip): out[f] = the mean over channels, rows and columns of
 *   S = ((2 ux uy + c1)(2 sxy + c2)) / ((ux^2 + uy^2 + c1)(sx + sy + c2)),   s.. = cov_norm * (E[..] - u. u.),
 * where ux, uy, E[x^2], E[y^2], E[xy] are the means of frame f of pred and gt under the separable window
 * taps (x) taps (HOST array of 2 * radius + 1 doubles, radius 0..5).  reflect == 0: the border is cropped, S exists
 * where the window fits (H - 2 radius rows, W - 2 radius columns: scikit-image's structural_similarity, whose crop equals
 * the window radius); reflect != 0: the images are padded as torch's "reflect" does (index -1 -> 1) and S exists at every
 * pixel (kornia's ssim).  Both images are read in place: element (x, y, channel, frame) of pred lies at
 * pred[x * s[0] + y * s[1] + channel * s[2] + frame * s[3]] with s = pred_strides4 (HOST array, in elements), likewise gt.
 * Moments and S are evaluated in float64 from the float32 inputs.  map: null, or (frames, channels, rows, columns) float32
 * receiving S.  partials: mnrf_ssim_blocks(H, W, frames, channels) doubles of workspace -- one per 32 x 16 tile of the H x W
 * image, channel and frame, an upper bound on what a launch writes for any radius and border rule (the output of a cropped
 * border is smaller and may take fewer tiles); 0 for a non-positive argument.  No atomics: deterministic, and
 * out[f] does not depend on the other frames.  H and W must hold a window, frames and channels must be positive. */
int64_t mnrf_ssim_blocks(int H, int W, int frames, int channels);
int mnrf_ssim(const float* pred, MNRF_HOST const int64_t* pred_strides4, const float* gt, MNRF_HOST const int64_t* gt_strides4, int H, int W,
              int channels, int frames, MNRF_HOST const double* taps, int radius, int reflect, double cov_norm, double c1, double c2,
              double* partials, float* out, float* map, void* stream);

/* ---- mesh extraction (extract_color_mesh.py): density grid, marching cubes, connected components, vertex colours.
 * csrc/mnrf_mesh.hip.  As everywhere: caller-owned buffers, no device state, arguments validated before the GPU is touched. */

/* The query points of the density volume, rows [start, start + count) of the reference's (N^3, 3) float32 tensor
 * (extract_color_mesh.py:146-152): numpy.linspace(lo, hi, N) per axis in float64 (i * ((hi - lo) / (N - 1)) + lo, the
 * last sample equal to hi), numpy.meshgrid(x, y, z) in its default "xy" order -- the flat index runs y, x, z from slow
 * to fast -- then the cast to float32.  Bit-identical to that construction.  out: (count, 3). */
int mnrf_grid_points(double x0, double x1, double y0, double y1, double z0, double z1, int n, int64_t start,
                     int64_t count, float* out, void* stream);
/* x = max(x, 0) in place (extract_color_mesh.py:185); a NaN stays a NaN. */
int mnrf_clamp_zero(float* x, int64_t n, void* stream);

/* Marching cubes over a C-ordered (nx, ny, nz) volume with welded vertices (one per crossed grid edge), in two phases so
 * that the caller can allocate exact sizes:
 *   blocks = mnrf_mc_blocks(nx, ny, nz);  mnrf_mc_count -> block_counts (blocks, 2) int32: per block of grid points in
 *   flat order, the crossed edges its points own (+x, +y, +z of each point) and the triangles of the cells it owns (a cell
 *   belongs to its lowest corner);  block_offsets = the EXCLUSIVE scan of block_counts along the blocks (the caller's; the
 *   totals are the mesh's vertex and triangle counts);  mnrf_mc_emit -> vertices (n_vertices, 3) in index coordinates of
 *   the volume and triangles (n_triangles, 3) int32.
 * Conventions: a corner is inside <=> value >= threshold; an edge is crossed <=> its ends differ; the vertex lies at
 * p0 + (threshold - s0) / (s1 - s0) from the edge's lower-index end p0; triangles are wound so that the geometric normal
 * points towards lower values.  No atomics: the output order is the flat order of the volume, two runs are bit-identical.
 * vertex_base: workspace of nx * ny * nz int32.  At most 2^30 grid points and 2^29 vertices.  Offsets that do not belong
 * to this volume never make the launch write outside [0, n_vertices) / [0, n_triangles). */
int64_t mnrf_mc_blocks(int nx, int ny, int nz);
int mnrf_mc_count(const float* volume, int nx, int ny, int nz, float threshold, int32_t* block_counts, void* stream);
int mnrf_mc_emit(const float* volume, int nx, int ny, int nz, float threshold, const int32_t* block_offsets,
                 int32_t* vertex_base, int64_t n_vertices, int64_t n_triangles, float* vertices, int32_t* triangles,
                 void* stream);
/* One row of the 256-case triangle table (HOST call, no GPU): up to five triangles as edge numbers, -1 terminated.
 * Corner c sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) and bit c of the case index is its inside flag; edge e
 * runs along axis e / 4 from the corner at offsets (k & 1, k >> 1), k = e % 4, along the two other axes in increasing
 * order.  The table is derived by scripts/gen_mc_table.py; ambiguous faces never join two inside corners. */
int mnrf_mc_table(int case_index, int8_t* out16);

/* Connected components of a triangle mesh by union-find over its vertices (hooking with an atomic min + pointer
 * jumping): mnrf_cc_init sets labels[v] = v; each mnrf_cc_step hooks along every triangle, flattens, and stores 1 into
 * *changed (device int32, zeroed by the caller) if it joined anything -- repeat until it stays 0; labels[v] is then the
 * smallest vertex of v's component.  mnrf_cc_count adds, per triangle, 1 to counts[label of its first vertex]
 * (counts: n_vertices int32, zeroed by the caller).  Triangles that index outside [0, n_vertices) are skipped. */
int mnrf_cc_init(int32_t* labels, int64_t n_vertices, void* stream);
int mnrf_cc_step(const int32_t* triangles, int64_t n_triangles, int32_t* labels, int64_t n_vertices, int32_t* changed,
                 void* stream);
int mnrf_cc_count(const int32_t* triangles, int64_t n_triangles, const int32_t* labels, int64_t n_vertices,
                  int32_t* counts, void* stream);

/* One view of the vertex colouring (extract_color_mesh.py:269-355).  mnrf_project_colors: project world-space vertices
 * with the HOST matrices w2c (3x4 float64, row-major: the inverse of the camera-to-world pose) and K = [[focal, 0, W/2],
 * [0, focal, H/2], [0, 0, 1]] in float64 (flip y/z, depth = z + 1e-5, pixel = float32(uv / depth) clipped to the image),
 * sample image (H, W, 3) uint8 bilinearly in float -> colors (n, 3), depth (n) float64, and the occlusion rays (n, 8) =
 * [origin, normalize(vertex - origin), near, far = depth].  mnrf_accumulate_colors: w = 0.1 / depth + (opacity <
 * occ_threshold), color_sum += colors * w, weight_sum += w (float64; a NaN opacity counts as 0, as numpy.nan_to_num does
 * the way the reference calls it). */
int mnrf_project_colors(const float* vertices, int64_t n_vertices, const uint8_t* image, int H, int W,
                        MNRF_HOST const double* w2c_host12, MNRF_HOST const float* origin_host3, float focal, float near, float* colors,
                        double* depth, float* rays, void* stream);
int mnrf_accumulate_colors(const float* colors, const double* depth, const float* opacity, float occ_threshold,
                           int64_t n_vertices, double* color_sum, double* weight_sum, void* stream);

/* Colouring along the vertex normals (extract_color_mesh.py --use_vertex_normal, lines 247-267 and 358-362).
 * mnrf_vertex_normals: normals (n_vertices, 3) float32 = for every vertex the sum, over the triangles (a, b, c) that hold
 * it, of the unnormalised (v_b - v_a) x (v_c - v_a) (float64 from the float32 vertices; so: area-weighted, direction by the
 * winding as given), normalised in float64 and cast.  A vertex whose sum is zero (no triangle, only degenerate ones) or that
 * shares a triangle with a non-finite vertex gets (0, 0, 1).  Deterministic and independent of the order of the triangles:
 * the components are accumulated as 64-bit integers (vector-memory integer atomics) in steps of 2^-k, k chosen on the device
 * from the largest cross-product component M of the mesh and the triangle count so that no sum can overflow; a step is at
 * most M * 2^(b - 61), 3 * n_triangles < 2^b.  scratch: mnrf_vertex_normals_scratch_bytes(n_vertices) bytes, 8-byte aligned
 * (zeroed by the call).  Triangles that index outside [0, n_vertices) are skipped.
 * mnrf_normal_rays: rays (n, 8) = [v - (n * near) * near_t, n, near, far] in float32, each operation rounded on its own.
 * mnrf_rgb_to_uint8: out[i] = the float32 product rgb[i] * 255 truncated towards zero (saturated to [0, 255], NaN -> 0). */
int64_t mnrf_vertex_normals_scratch_bytes(int64_t n_vertices);
int mnrf_vertex_normals(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                        void* scratch, float* normals, void* stream);
int mnrf_normal_rays(const float* vertices, const float* normals, int64_t n_vertices, float near, float far, float near_t,
                     float* rays, void* stream);
int mnrf_rgb_to_uint8(const float* rgb, int64_t n, uint8_t* out, void* stream);

/* ---- the ray bank (csrc/mnrf_bank.hip): training batches from frames that stay on the device as decoded bytes
 * (datasets/blender.py:51-108, 159-168, 191-204 without the 48 B per ray of host float arrays and without the DataLoader).
 * All arrays are DEVICE memory of the caller; the struct itself is host memory, read during the call.  N = slots * H * W;
 * a global index g addresses slot g / (H*W) and pixel g % (H*W), a slot being frame `slot`, or frames[slot] when a frame
 * list is given (the reference's *_wmask subset: slots counts its entries; without a list slots == n_frames). */
typedef struct {
    const float* poses;       /* (n_frames, 3, 4) camera-to-world */
    const uint8_t* images;    /* (n_frames, H, W, channels) */
    const int8_t* masks;      /* (n_frames, H, W): -1 = no ground-truth mask for the frame, 0, 1 */
    const int32_t* frames;    /* (slots) frame numbers, or null */
    int n_frames, H, W, channels, slots;
    float focal, near, far;
} MnrfBank;
/* Row k of the outputs for pixel indices[k] (device int64), or for start + k when indices is null (start .. start + n must
 * lie inside the bank: how a whole frame is read).  rays (n, 8): bit-identical to the same pixel of mnrf_generate_rays;
 * rgbs (n, 3): float(v) / 255.0f, with four channels rgb * a + (1 - a) as separate fp32 operations; mirror_mask (n): the
 * int8 as a float; valid_mask (n) bytes: last channel > 0.  Any output may be null.  An index outside [0, N), or a frame
 * number outside [0, n_frames), reads nothing: its row is NaN (valid 0).  n == 0 is a no-op. */
int mnrf_bank_gather(const MnrfBank* bank, const int64_t* indices, int64_t start, int64_t n, float* rays, float* rgbs,
                     float* mirror_mask, uint8_t* valid_mask, void* stream);
/* The same outputs for the `batch` pixels of one step of a shuffled stream that visits every pixel once per epoch.  Lane l of
 * `rank` in `world` at step s = step + (step_dev ? *step_dev : 0) (step_dev: device int64, so that a captured graph can
 * replay the draw and advance the word) takes stream position p = (s * world + rank) * batch + l, epoch = p / N, i = p % N
 * and pixel g = perm(seed, epoch)(i); indices_out (batch) int64 receives g when not null.  perm is a six-round balanced
 * Feistel network over 2 * ceil(max(2, bit_length(N - 1)) / 2) bits with cycle walking; the mixer and the key schedule are
 * stated in the header comment of csrc/mnrf_bank.hip and are part of the contract: a (seed, step, rank, world, batch)
 * names the same pixels on every build.  N >= 2^32 is refused (before any pointer is looked at).  batch == 0 is a no-op. */
int mnrf_bank_draw(const MnrfBank* bank, uint64_t seed, int64_t step, const int64_t* step_dev, int rank, int world,
                   int64_t batch, float* rays, float* rgbs, float* mirror_mask, uint8_t* valid_mask, int64_t* indices_out,
                   void* stream);

/* ---- the output stage of eval.py (csrc/mnrf_frames.hip; eval.py:743-978, utils/visualization.py:10-23, 208-221): the
 * 8-bit images of a rendered frame from its float32 maps, which stay where batched_inference left them.  Two launches per
 * frame (extrema, finish), no host read between or after them.  The expressions, the cast and the reduction are stated in
 * the header comment of csrc/mnrf_frames.hip; every byte is what numpy gives for the reference's expression.
 * A null map or a null image skips that image.  Every image is (n, 3) bytes, the reference's (H, W, 3). */
typedef struct {
    const float* rgb;                  /* (n, 3) */
    const float* mirror_mask;          /* (n) */
    const float* depth;                /* (n) */
    const float* depth_reflect;        /* (n); its image also needs mirror_mask */
    const float* surface_normal;       /* (n, 3) */
    const float* surface_normal_grad;  /* (n, 3) */
    const float* x_surface;            /* (n, 3) */
} MnrfFrameMaps;
typedef struct {
    uint8_t* rgb;
    uint8_t* mirror_mask;
    uint8_t* depth;
    uint8_t* depth_reflect;
    uint8_t* surface_normal;
    uint8_t* surface_normal_grad;
    uint8_t* x_surface;
} MnrfFrameImages;
/* Sizes, in floats, of a frame's stats block and of the split-wide running block.
 * The stats block: [0], [1] min and max of nan_to_num(depth); [2], [3] of nan_to_num(depth_reflect); [4], [5] of x_surface
 * over its three channels (a NaN makes both NaN, as torch.min does); the rest is the reduction's own state, which must be
 * ZERO before the first launch on a block and is left zero by every launch.  A null map leaves NaN in its entries.
 * The running block: min and max of the raw depth, then of the raw reflected depth, over every frame folded into it: a
 * frame's np.min / np.max replaces the entry when it is smaller / larger (eval.py:776-785); a frame that holds a NaN has NaN
 * extremes and changes nothing, an infinity counts.  The caller resets the block to (+inf, -inf, +inf, -inf). */
int mnrf_frame_stats_floats(void);
int mnrf_split_extrema_floats(void);
/* The extremes of one frame into `stats`, and its raw depth extremes folded into `running` (null: not folded).  Any map may
 * be null.  Deterministic: integer atomics on an order-preserving image of the floats.  n == 0 is a no-op. */
int mnrf_frame_extrema(const float* depth, const float* depth_reflect, const float* x_surface, int64_t n, float* stats,
                       float* running, void* stream);
/* Every image whose map and output are both given, in one launch; `stats` as the extrema launch left it on the same stream;
 * table: (256, 3) bytes on the device, the colour of depth index k in the channel order it is to be stored in (required
 * when a depth image is asked for).  The maps are only read. */
int mnrf_frame_finish(const MnrfFrameMaps* maps, const MnrfFrameImages* images, int64_t n, const float* stats,
                      const uint8_t* table, void* stream);
/* The depth colour map of a stack of resident maps, depth (frames, n) -> out (frames, n, 3), in one launch.  extrema: two
 * device floats (vmin, vmax) for every frame -- a pair of the running block for save_depth_unified_normalization -- or null
 * for each frame's own extremes, which one more launch then reduces into `stats` (frames stats blocks, zero before first
 * use).  mask (frames, n) or null: the reflected variant, the colour multiplied by clip(mask, 0, 1). */
int mnrf_depth_colormap(const float* depth, const float* mask, int64_t frames, int64_t n, const float* extrema, float* stats,
                        const uint8_t* table, uint8_t* out, void* stream);

/* ---- the validation panel (csrc/mnrf_frames.hip; utils/visualization.py:26-184 with add_text=False): the (n_tiles, 3, H, W)
 * float32 stack the reference logs as val/GT_pred_depth, from the maps of one validation frame, read in place.  Two launches:
 * the extrema launch reduces min and max of every GLOBAL and every DEPTH tile, the write launch produces the whole stack,
 * every element once.  Each tile is the reference's expression in single fp32 operations (header comment of the kernels).
 * maps: host array of n_tiles device pointers; kinds: one MNRF_PANEL_* per tile.  COPY, NORMAL and GLOBAL read an (H W, 3)
 * map, MASK and DEPTH an (H W) map.  stats: n_tiles slots of mnrf_val_panel_stats_floats() floats, tile t's at
 * [t * that]: [0] min, [1] max, the rest the reduction's state, ZERO before the first launch and left zero; only GLOBAL and
 * DEPTH slots are touched, and stats may be null when there is no such tile.  At most 32 tiles.  n_tiles == 0 or H W == 0 is
 * a no-op; a null array, a null map, a negative size or an unknown kind is refused before anything is launched. */
#define MNRF_PANEL_COPY 0     /* out[c][p] = map[p][c] */
#define MNRF_PANEL_MASK 1     /* out[c][p] = map[p] */
#define MNRF_PANEL_NORMAL 2   /* out[c][p] = (map[p][c] + 1) / 2 */
#define MNRF_PANEL_GLOBAL 3   /* visualize_rgb_map_global: (map - min) / (max - min) over the whole map; ones when min == max */
#define MNRF_PANEL_DEPTH 4    /* visualize_depth with the map's own extremes, coloured through `table`, / 255 */
int mnrf_val_panel_stats_floats(void);
int mnrf_val_panel_extrema(const float* const* maps, MNRF_HOST const int* kinds, int n_tiles, int H, int W, float* stats,
                           void* stream);
/* table: (256, 3) bytes on the device as for mnrf_frame_finish (required with a DEPTH tile); stats as the extrema launch
 * left it on the same stream; out: (n_tiles, 3, H, W) floats. */
int mnrf_val_panel_write(const float* const* maps, MNRF_HOST const int* kinds, int n_tiles, int H, int W, const float* stats,
                         const uint8_t* table, float* out, void* stream);

/* ---- the ingest step of the ray bank (csrc/mnrf_resample.hip; datasets/real_arkit.py:236-237, 251-264): decoded frames are
 * resized on the device.  The arithmetic is Pillow's 8-bit resampler, stated in the header comment of csrc/mnrf_resample.hip:
 * a pass along x into `tmp`, rounded to 8 bits, then a pass along y; a pass whose sizes agree is not run.  src (frames, src_h,
 * src_w, channels), dst (frames, dst_h, dst_w, channels), channels 3 or 4; four channels are RGBA, premultiplied at the first
 * pass's loads and divided out at the last pass's stores.  Per resized axis the caller hands in the tables data.lanczos_taps
 * makes on the host: bounds (out, 2) int32 (first source sample, count) and taps (ksize, out) int32 (22 fraction bits, tap k
 * of output i at [k * out + i]); the tables of a pass that is not run may be null.  Every window is clamped to the source extent
 * and to ksize before use.  tmp: (frames, src_h, dst_w, channels) bytes of the caller's, needed when both passes run (the size
 * below; 0 when at most one pass runs, -1 for sizes the call would refuse).  Refused: sizes < 1, channels other than 3 or 4,
 * null pointers, and src and dst sizes that agree on both axes (nothing to resample: the caller copies). */
int64_t mnrf_resample_tmp_bytes(int64_t frames, int src_h, int src_w, int dst_h, int dst_w, int channels);
int mnrf_resample_u8(const uint8_t* src, int64_t frames, int src_h, int src_w, int channels, uint8_t* dst, int dst_h, int dst_w,
                     const int32_t* taps_x, const int32_t* bounds_x, int ksize_x, const int32_t* taps_y,
                     const int32_t* bounds_y, int ksize_y, uint8_t* tmp, void* stream);
/* A mirror mask at its native depth to the bank's int8: src (frames, src_h, src_w) samples of 1 or 2 bytes (native byte
 * order), dst (frames, dst_h, dst_w).  Output (y, x) picks source (min(floor(y * (src_h / dst_h)), src_h - 1), the same in x),
 * the quotient and the product in double (cv2's INTER_NEAREST rule as data._resize_nearest states it); an 8-bit sample >= 128
 * gives 1, a 16-bit sample > 0 gives 1, anything else 0. */
int mnrf_mask_nearest(const void* src, int sample_bytes, int64_t frames, int src_h, int src_w, int8_t* dst, int dst_h, int dst_w,
                      void* stream);

/* ---- the D-NeRF object field (csrc/mnrf_dnerf.hip; models/d_nerf/run_dnerf_helpers.py:70-253, DirectTemporalNeRF with D = 8,
 * W = 256, skips = [4], multires 10 / 4, use_viewdirs): a deformation net (_time.0..7, _time_out) that moves a point by dx at
 * time t, and a canonical NeRF (_occ) evaluated on the encoding of x + dx.  fp32 matrix instructions only.
 *
 * The packed image: `params` is a HOST array of MNRF_DNERF_N_PARAMS device pointers in state_dict order -- _occ.pts_linears.0..7,
 * _occ.views_linears.0, _occ.feature_linear, _occ.alpha_linear, _occ.rgb_linear, _time.0..7, _time_out, weight then bias each
 * (nn.Linear layout (out,in) row-major).  The image holds no device state: launches only read it. */
#define MNRF_DNERF_N_PARAMS 42
#define MNRF_DNERF_SIGMA_ONLY 1u   /* stop in front of the colour branch (the coarse pass): rgb is not written */
#define MNRF_DNERF_RAW_RGB 2u      /* rgb without the sigmoid (the module's forward; raw2outputs applies it) */
#define MNRF_DNERF_CANONICAL 4u    /* t == 0 with zero_canonical (run_dnerf_helpers.py:147-148): the deformation net is not
                                    * evaluated, dx is written as zeros */
int64_t mnrf_dnerf_packed_floats(void);
int mnrf_dnerf_pack_weights(const float* const* params, float* packed, void* stream);
/* DirectTemporalNeRF.forward on B samples at ONE time t.  Positions, view encoding and null outputs as in mnrf_field_forward:
 * `xyz` rows or o + d*z from `rays` (n_rays, 8) and `z_vals` (n_rays, spr) (separate multiply and add), `dir_emb` rows of 27
 * floats with row index sample / spr (not read with MNRF_DNERF_SIGMA_ONLY).  The 21 channels of the time encoding are the same
 * for every sample: their product with _time.0's last 21 columns is added to that layer's bias once per workgroup.
 * Outputs (null = skip): sigma (B) raw, rgb (B,3) after the sigmoid (raw with MNRF_DNERF_RAW_RGB), dx (B,3).  The canonical
 * trunk sees the encoding of x + dx (one fp32 add).  Rows past B are not written. */
int mnrf_dnerf_forward(const float* packed, unsigned flags, int64_t B, const float* xyz, int64_t xyz_stride, const float* rays,
                       const float* z_vals, int spr, const float* dir_emb, int64_t dir_stride, float t, float* sigma, float* rgb,
                       float* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MNRF_H */
