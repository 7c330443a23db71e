/*
 * fp_amd.h -- C ABI of the MI355X-native render-and-compare hot path (libfp_amd.so).
 *
 * The reference (NVlabs/FoundationPose) has no FFI boundary for this path: it is plain
 * Python calling nvdiffrast / kornia / warp / torch.  This header is
 * therefore the boundary *underneath* the preserved Python API; every entry point cites the
 * reference lines it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / STL types.
 *   - return 0 on success, a negative fp_status otherwise; fp_last_error() gives the message
 *     (thread-local).
 *   - pointers marked [dev] are device (HBM) pointers owned by the caller; [host] are host
 *     pointers read before the call returns.  No entry point allocates, frees or synchronises;
 *     all work is enqueued on `stream` (a hipStream_t), so sequences are hipGraph-capturable.
 *   - images are row-major; poses are row-major 4x4 float32 `ob_in_cam` (OpenCV camera).
 */
#ifndef FP_AMD_H
#define FP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  FP_OK = 0,
  FP_ERR_INVALID_ARG = -1,
  FP_ERR_WORKSPACE = -2,
  FP_ERR_LAUNCH = -3,
  FP_ERR_UNSUPPORTED = -4
} fp_status;

/* flags for fp_render_crops / fp_warp_crops */
#define FP_FLAG_NORMALIZE_XYZ 1 /* cfg['normalize_xyz'] (h5_dataset.py:95-101,151-156) */
#define FP_FLAG_OUT_F16 2       /* write the network tensor (A / B) as fp16 instead of fp32 */

/* fp_warp_crops mode */
#define FP_MODE_REFINE 0 /* predict_pose_refine.py:63,72 + PairH5Dataset.transform_batch */
#define FP_MODE_SCORE 1  /* predict_score.py:89-90 + TripletH5Dataset.transform_depth_to_xyzmap */

/* fp_pose_update rot_rep / trans_rep */
#define FP_ROT_AXIS_ANGLE 0
#define FP_ROT_6D 1
#define FP_TRANS_TRACKNET 0 /* cfg['trans_rep'] = 'tracknet' (the released configuration), predict_pose_refine.py:195-199 */
#define FP_TRANS_DEEPIM 1   /* 'deepim': crop-space shift of the projected centre + depth ratio, predict_pose_refine.py:201-215 */
#define FP_TRANS_RAW 2      /* any other trans_rep: the plain `else` branch (:217-218), the raw output (x diameter/2 if normalize_xyz) */

/* integer z-buffer definition; shared with oracle/fp_oracle.c */
#define FP_SUBPIXEL_BITS 4
#define FP_ZBUF_STEPS_PER_METRE 1048576 /* 2^20 */
#define FP_ZBUF_EMPTY 0xFFFFFFFFu

typedef struct fp_mesh fp_mesh; /* opaque: device pointers + sizes of one object's mesh tensors */
typedef struct fp_mesh_set fp_mesh_set; /* opaque: M mesh descriptors in one device table (several objects per call) */

const char* fp_last_error(void);
/* ABI version of the library = FP_AMD_ABI_VERSION of the header it was built from; a binding compares the two at load time
 * (foundationpose_amd/_lib.py does and refuses a mismatch).  History of breaks that kept a symbol's name:
 *   200 -> 210 (round 4 / 5): fp_linear_layernorm_fwd takes the FRAGMENT-PACKED weight (fp_pack_linear512_f16) and requires K = 512;
 *                             a caller that still passes the nn.Linear-layout weight gets FP_OK and garbage -- check the version.
 *   210 -> 211 (round 5): + fp_igemm_f16_splitk_fwd / fp_igemm_splitk_workspace_bytes (additions only).
 *   211 -> 212 (round 5): fp_igemm_epilogue grew by one member at its end (w_tiles); + fp_pack_conv3x3_tiles_f16.
 *   212 -> 213 (round 6): w_tiles is read only when flags has FP_IGEMM_HAS_W_TILES (a 212 caller that sets w_tiles without the bit
 *                         gets the plain weight path: correct, slower); fp_igemm_f16_splitk_fwd refuses w_tiles instead of ignoring it;
 *                         fp_linear_layernorm_fwd takes the row stride of x16 (new argument before the stream);
 *                         + fp_encoder_tail_mean_fwd / fp_encoder_tail_workspace_bytes.
 *   213 -> 214: several objects per call (additions only): + fp_mesh_set_create / fp_mesh_set_destroy /
 *               fp_mesh_set_workspace_bytes, fp_render_crops_multi, fp_crop_windows_multi, fp_warp_crops_multi, fp_pose_update_multi.
 *   214 -> 215: + fp_attention_segments_f16_fwd (addition only): attention over ragged sequences (several objects' hypotheses).
 *   215 -> 216: several views per call (additions only): + fp_crop_windows_views, fp_render_crops_views, fp_warp_crops_views,
 *               fp_pose_update_views, fp_depth_erode_frames, fp_depth_bilateral_frames, fp_depth_to_xyz_frames.
 *   216 -> 217: registration in several views per call (additions only): + fp_mask_depth_stats, fp_replicate_segments_f16.
 *   217 -> 218: + fp_depth_agreement (addition only): per-hypothesis depth agreement of a rendered pose with the observed frame.
 *   218 -> 219: + fp_pose_errors, fp_pose_errors_workspace_bytes (additions only): ADD, ADD-S and symmetry-aware errors of pose batches.
 *   219 -> 220: + fp_vsd_counts, fp_mspd (additions only): the pixel counts of BOP's visible surface discrepancy and its maximum
 *               symmetry-aware projection distance, for pose batches.
 *   220 -> 221: + fp_tsdf_integrate, fp_tsdf_count_triangles, fp_tsdf_emit_triangles (additions only): an object's mesh from posed
 *               RGB-D reference views (truncated-signed-distance fusion and marching tetrahedra).
 *   221 -> 222: + FP_IGEMM_MFMA_16X16X32 / FP_IGEMM_MFMA_32X32X16 (additions only; an older library refuses the bits as unknown flags).
 *   222 -> 223: + fp_texture_bake (addition only): a texture atlas for a fused mesh from its posed RGB-D reference views.
 *   223 -> 224: + fp_raster_lds_bytes, fp_conv3x3_sw_lds_bytes (additions only): the LDS a workgroup of the rasteriser and of the
 *               3x3 convolution asks for at launch.
 *   224 -> 225: + FP_IGEMM_EPILOGUE_GENERIC (addition only; an older library refuses the bit as an unknown flag).
 *   225 -> 226: + fp_icp_point_plane, fp_icp_workspace_bytes (additions only): one Gauss-Newton step of point-to-plane ICP per
 *               hypothesis, the render of a pose against the observed depth.
 *   226 -> 227: + FP_IGEMM_DIRECT_STORE / FP_IGEMM_W_TILES_DIRECT, fp_pack_conv3x3_tiles_direct_f16 (additions only; an older library
 *               refuses the bits as unknown flags).
 *   227 -> 228: + fp_tsdf_raycast (addition only): depth, points, normals and colours of a TSDF volume's zero surface at any pose, in
 *               the layout fp_icp_point_plane and fp_depth_agreement read.
 *   228 -> 229: + fp_tsdf_label_components (addition only): the face-connected components of a volume's surface cubes and their
 *               triangle counts, for dropping floaters at extraction.
 *   229 -> 230: fp_crop_windows, fp_render_crops, fp_warp_crops and fp_pose_update CHANGED SIGNATURE IN PLACE: each now takes the camera
 *               as K or as Ks / view / V and the object as mesh_diameter or as diameters / obj / M (render: mesh or set) in one argument
 *               list.  REMOVED: fp_crop_windows_multi, fp_crop_windows_views, fp_render_crops_multi, fp_render_crops_views,
 *               fp_warp_crops_multi, fp_warp_crops_views, fp_pose_update_multi, fp_pose_update_views.  A caller of the four base names
 *               built against an older header passes the wrong arguments: gate on fp_version().
 *   230 -> 231: + fp_mesh_point_distance, fp_mesh_point_distance_workspace_bytes (additions only): the exact distance from points to
 *               the surface of a triangle mesh, with the nearest face and the closest point.
 *   231 -> 232: + fp_mesh_transform_residuals, fp_mesh_transform_residuals_workspace_bytes (additions only): how far each of T
 *               candidate transforms moves a mesh's surface samples off the surface, for detecting its rotational symmetries.
 *   232 -> 233: + fp_mesh_icp_step, fp_mesh_icp_workspace_bytes (additions only): one Gauss-Newton step of point-to-plane ICP for each
 *               of T candidate transforms of a mesh's surface samples against another mesh, for registering one onto the other.
 *   233 -> 234: + fp_mesh_pseudonormals, fp_mesh_signed_distance, fp_mesh_signed_distance_workspace_bytes, fp_mesh_penetration,
 *               fp_mesh_penetration_workspace_bytes (additions only): which side of a closed mesh a point is on, and how far T
 *               placements of a point set reach into it.
 *   234 (kept): + fp_pack_linear512_direct_f16, fp_linear512_flags_f16_fwd (additions only): the in_proj kernel that stores its tiles
 *               from the accumulators, and the flags that select it.  No signature and no behaviour of an existing symbol changes, and
 *               tests/test_mesh_signed_host.py pins the number; a binding that needs the new symbols finds an older library by their
 *               absence.
 *   234 (kept): + fp_mesh_grid_count, fp_mesh_grid_fill, fp_mesh_grid_fill_workspace_bytes, fp_mesh_grid_point_distance,
 *               fp_mesh_grid_signed_distance and the struct fp_mesh_grid (additions only): a uniform grid over a mesh's triangles and
 *               the two point queries answered from it with the brute force's bits.  The number stays for the same reason.
 *   234 (kept): + fp_mesh_grid_transform_residuals, fp_mesh_grid_icp_step, fp_mesh_grid_penetration (additions only): the three
 *               batched transform queries answered from the same grid with the brute force's bits.  The number stays for the same
 *               reason: tests/test_mesh_signed_host.py pins it, and a binding finds an older library by the symbols' absence.
 *   234 (kept): + fp_mesh_ray_cast, fp_mesh_ray_cast_workspace_bytes (additions only): what a ray hits first on a triangle mesh, by
 *               brute force on the scan's own tile.  The number stays for the same reason. */
#define FP_AMD_ABI_VERSION 234
int fp_version(void);

/* Utils.py:104-130 make_mesh_tensors: records caller-owned device tensors.
 * pos/nrm (V,3) f32, faces (T,3) i32; either {tex (Ht,Wt,3) f32 in [0,1], uv (V',2) f32 with v already
 * flipped (Utils.py:117), uv_idx (T,3) i32 or NULL => faces} or {vcol (V,3) f32 in [0,1]}. */
int fp_mesh_create(const float* pos /*dev*/, const float* nrm /*dev*/, const int32_t* faces /*dev*/,
                   const float* uv /*dev|NULL*/, const int32_t* uv_idx /*dev|NULL*/,
                   const float* tex /*dev|NULL*/, const float* vcol /*dev|NULL*/, int V, int T, int Ht,
                   int Wt, fp_mesh** out);
void fp_mesh_destroy(fp_mesh* mesh);

/* Several objects per call: a mesh set holds M mesh descriptors (fp_mesh_create) in one device table, for fp_render_crops (see "The
 * crop stage" below).  fp_mesh_set_create is a SETUP call: it allocates the device table and copies the descriptors synchronously (the
 * per-frame entry points copy nothing, so they can be captured in a hipGraph).  The set refers to the meshes' tensors, it does not own
 * them; the fp_mesh handles themselves may be destroyed after the call.  V and T of every mesh: 1..FP_MESH_SET_MAX_ELEMS. */
#define FP_MESH_SET_MAX_ELEMS (1 << 26)
int fp_mesh_set_create(const fp_mesh* const* meshes /*host M*/, int M, fp_mesh_set** out);
void fp_mesh_set_destroy(fp_mesh_set* set);
/* fp_workspace_bytes for the set's largest V and largest T (so the lists are 32-bit when any mesh has T > 65535) */
size_t fp_mesh_set_workspace_bytes(const fp_mesh_set* set, int N, int oh, int ow);

/* Utils.py:359-395 erode_depth (+ kernel) */
int fp_depth_erode(const float* depth /*dev H,W*/, float* out /*dev*/, int H, int W, int radius,
                   float depth_diff_thres, float ratio_thres, float zfar, void* stream);
/* Utils.py:304-356 bilateral_filter_depth (+ kernel) */
int fp_depth_bilateral(const float* depth /*dev*/, float* out /*dev*/, int H, int W, int radius,
                       float zfar, float sigmaD, float sigmaR, void* stream);
/* Utils.py:399-417 depth2xyzmap (f64_internal=1, numpy promotion) / :420-438 depth2xyzmap_batch (0) */
int fp_depth_to_xyz(const float* depth /*dev H,W*/, const double* K /*host 9*/, float zfar,
                    int f64_internal, float* xyz /*dev H,W,3*/, int H, int W, void* stream);

/* Several views per call: the batched ingest of V frames of one size, one launch per stage over a (V,H,W) stack (frame f of every
 * output = what the single-frame entry point computes on frame f of the input, bit for bit).  1 <= V <= 65535.
 * fp_depth_to_xyz_frames reads the intrinsics of frame f from Ks[f] (dev V,9 f64: the values fp_depth_to_xyz takes on the host). */
int fp_depth_erode_frames(const float* depth /*dev V,H,W*/, float* out /*dev V,H,W*/, int H, int W, int V, int radius,
                          float depth_diff_thres, float ratio_thres, float zfar, void* stream);
int fp_depth_bilateral_frames(const float* depth /*dev V,H,W*/, float* out /*dev V,H,W*/, int H, int W, int V, int radius,
                              float zfar, float sigmaD, float sigmaR, void* stream);
int fp_depth_to_xyz_frames(const float* depth /*dev V,H,W*/, const double* Ks /*dev V,9*/, float zfar, int f64_internal,
                           float* xyz /*dev V,H,W,3*/, int H, int W, int V, void* stream);

/* estimater.py:137-156 guess_translation and the "fewer than 4 valid depths" test of register() (estimater.py:164-166), for M masks
 * over a (V,H,W) f32 depth stack in one launch: mask m ((M,H,W) uint8, nonzero = inside) lies on frame view[m] (dev M int32; NULL
 * allowed only for V == 1).  out (dev M,8 int32) per mask: {v0, v1, u0, u1, n, lo, hi, 0} -- the mask's bounding box (rows v0..v1,
 * columns u0..u1; all -1 for an empty mask), the count n of its valid depths (d >= min_depth), and lo / hi as float bits: the
 * (n-1)//2-th and n//2-th smallest valid depths, the elements torch.sort puts there (exact; NaN when n == 0).  A view index outside
 * 0..V-1 reads nothing and reports an empty mask.  min_depth must be positive and finite.  No allocation, no synchronisation. */
int fp_mask_depth_stats(const float* depth /*dev V,H,W*/, const uint8_t* masks /*dev M,H,W*/, const int32_t* view /*dev M|NULL*/,
                        int V, int M, int H, int W, float min_depth, int32_t* out /*dev M,8*/, void* stream);

/* How well each pose agrees with the observed depth (the signal that a track is lost), for N hypotheses in one launch.  For hypothesis n
 * and crop pixel (i, j): z_r = depth_crops[n, j, i], the render's depth at the pose (fp_render_crops* with these tf_to_crops' windows;
 * 0 where it draws nothing), and z_o = the z of the texel of frame view[n]'s xyz map that the REFINE warp reads for that pixel (the
 * nearest texel through the inverse of tf_to_crops[n]; 0 outside the frame) -- bit for bit the z channel of fp_warp_crops* in
 * FP_MODE_REFINE without FP_FLAG_NORMALIZE_XYZ called with the pose's translation zeroed.  counts[n] (int32 x 4), every difference in
 * f32:  [0] model  = pixels with z_r > 0;
 *       [1] valid  = model pixels with z_o >= 0.001 (the REFINE threshold);
 *       [2] agree  = valid pixels with fabsf(z_o - z_r) <= tol;
 *       [3] behind = valid pixels with z_o - z_r > tol: the sensor sees past the model's surface (free space violated).
 * valid - agree - behind (not stored) = pixels where something lies in front of the model (an occlusion).  tol is absolute, in the
 * depth's unit (metres).  The counts are zeroed on the stream first (no host synchronisation: graph-capturable) and summed with integer
 * atomics: exact, the same on every replay.  xyz_map is a (V,H,W,3) stack, view a per-hypothesis index (dev N int32; NULL allowed only
 * for V == 1); an index outside 0..V-1 reads nothing (valid = agree = behind = 0).  N == 0 does nothing.  Argument errors
 * (FP_ERR_INVALID_ARG): NULL tensors, oh / ow / H / W / V below 1, more than 2^20 crop pixels, N outside 0..65535, view NULL with
 * V > 1, tol negative or not finite. */
int fp_depth_agreement(const float* depth_crops /*dev N,oh,ow*/, const float* xyz_map /*dev V,H,W,3*/, const float* tf_to_crops /*dev N,9*/,
                       const int32_t* view /*dev N|NULL*/, int V, int H, int W, int N, int oh, int ow, float tol,
                       int32_t* counts /*dev N,4*/, void* stream);
/* Polish poses against the observed depth: ONE Gauss-Newton step of point-to-plane ICP for each of N hypotheses, in two launches.
 * Defined to the float32 operation.  Per crop pixel (i, j) of hypothesis n, all in float32, one rounding per operation, every 3-term
 * sum as (a0*b0 + a1*b1) + a2*b2:
 *   p = xyz_crops[n, j, i], m = normal_crops[n, j, i]: the camera-frame point and unit normal fp_render_crops* writes at poses_in[n]
 *       through these tf_to_crops' windows (without FP_FLAG_NORMALIZE_XYZ; 0 where it draws nothing);
 *   model = p.z > 0 && m.m > 0;
 *   q = the texel of frame view[n]'s xyz map that fp_depth_agreement reads for that pixel (the nearest texel through the inverse of
 *       tf_to_crops[n]), all three channels; (0, 0, 0) outside the frame or for a view index outside 0..V-1: nothing is read there;
 *   valid = model && q.z >= 0.001f;   e = q - p;   pair = valid && e.e <= max_dist * max_dist (the product in float32; a NaN anywhere
 *       makes a comparison false, so the pixel is no pair);
 *   r = m.e;   a = p - c with c = (poses_in[n][3], [7], [11]);   J = (a1*m2 - a2*m1, a2*m0 - a0*m2, a0*m1 - a1*m0, m0, m1, m2).
 * The step moves the model as p' = c + dR(w) (p - c) + v: it rotates about the pose's own origin (the convention of
 * egocentric_delta_pose_to_pose), so J.x ~ r with x = (w, v).
 * Per hypothesis, float64: A = sum J^T J (its 21 upper entries), b = sum J^T r, sum r*r and the pair count, over the pairs.  Each term is
 * the product of the two float32 values widened to double (exact).  The sums run over chunks of 256 consecutive crop pixels (pixel
 * j * ow + i), inside a chunk over 4 waves of 64: within a wave by the xor tree (s += s of lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; a pixel
 * that is no pair adds +0), the waves in index order, then the chunks in index order starting from +0.  The order depends on (oh, ow)
 * alone and there are no floating-point atomics: row n has the same bits alone, in any batch and on every replay.
 * Solve, float64, without contraction: A_l = A + damping * diag(A) (A_l[j][j] = A[j][j] + damping * A[j][j]); LDL^T without pivoting,
 * for j = 0..5:  v_k = L[j][k] * d[k] and s = A_l[j][j], s = s - L[j][k] * v_k for k = 0..j-1 in order, d[j] = s;  for i = j+1..5:
 * u = A[j][i], u = u - L[i][k] * v_k for k = 0..j-1 in order, L[i][j] = u / d[j].  Forward: y[i] = b[i], y[i] = y[i] - L[i][k] * y[k]
 * for k = 0..i-1.  Diagonal: z[i] = y[i] / d[i].  Back, i = 5..0: x[i] = z[i], x[i] = x[i] - L[k][i] * x[k] for k = i+1..5 in order.
 * status: 2 when a value of the poses_in row (all 16) is not finite; else 1 when pairs < min_pairs; else 2 when a pivot d[j] is <= 0 or
 * not finite or a component of x is not finite; else 0.  For status != 0, x = 0 and the poses_out row is the poses_in row bit for bit.
 * Pose update, float64: th = sqrt((w0*w0 + w1*w1) + w2*w2); dR = I + [w]x below th = 1e-12, else with k = w / th, c = cos th, s = sin th:
 * dR = c I + s [k]x + (1 - c) k k^T (Rodrigues);  R' = dR * R_in (each entry (dR[i][0]*R[0][j] + dR[i][1]*R[1][j]) + dR[i][2]*R[2][j]),
 * t' = t_in + v, each rounded once to float32; row 3 is copied.
 * system[n] (float64 x 40): [0..20] A's upper triangle row-major, [21..26] b, [27] sum r*r, [28] pairs, [29] status, [30..35] x,
 * [36..39] 0.  The sums are reported whatever the status.  poses_out may be NULL (the system alone); poses_in and poses_out must not
 * overlap.  No allocation, no host synchronisation, no memset (graph-capturable); nothing is written outside system, poses_out and
 * workspace (fp_icp_workspace_bytes(N, oh, ow) bytes, 8-byte aligned; 0 for N <= 0).  N == 0 does nothing.  Argument errors
 * (FP_ERR_INVALID_ARG): NULL tensors with N > 0, oh / ow / H / W / V below 1, more than 2^20 crop pixels, N outside 0..65535, view NULL
 * with V > 1, max_dist or damping negative or not finite, min_pairs < 6, overlapping pose tables, a workspace that is too small or
 * misaligned. */
size_t fp_icp_workspace_bytes(int N, int oh, int ow);
int fp_icp_point_plane(const float* xyz_crops /*dev N,oh,ow,3*/, const float* normal_crops /*dev N,oh,ow,3*/,
                       const float* xyz_map /*dev V,H,W,3*/, const float* tf_to_crops /*dev N,9*/,
                       const int32_t* view /*dev N|NULL*/, int V, int H, int W, const float* poses_in /*dev N,16*/,
                       int N, int oh, int ow, float max_dist, double damping, int min_pairs,
                       double* system /*dev N,40*/, float* poses_out /*dev N,16|NULL*/,
                       void* workspace, size_t workspace_bytes, void* stream);
/* How far each of N poses is from its ground truth, in the units the field reports: out[n] = {add, adds, add_sym, mssd} (float64,
 * metres).  flags selects the columns (a column that is not selected is NaN): */
#define FP_ERR_ADD 1  /* add: mean distance of corresponding model points */
#define FP_ERR_ADDS 2 /* adds: mean distance of each ground-truth point to the nearest predicted point (P x P pairs per pose) */
#define FP_ERR_SYM 4  /* add_sym and mssd: the minimum over the symmetry set of the mean / of the maximum corresponding distance (BOP) */
/* Definition (poses are taken as rigid).  Pose n has ground truth g = gt_index[n] (NULL: g = 0 for G == 1, g = n for G == N).
 *  - T = inv(pose_n) * gt_g in float64, the inverse as [R^T | -R^T t], every 3-term sum as (a0*b0 + a1*b1) + a2*b2:
 *    T.R[i][j] = (Rp[0][i]*Rg[0][j] + Rp[1][i]*Rg[1][j]) + Rp[2][i]*Rg[2][j],  T.t[i] = (Rp[0][i]*d0 + Rp[1][i]*d1) + Rp[2][i]*d2 with
 *    d = t_g - t_p.  For symmetry s, T_s = T * S_s: T_s.R[i][j] = (T.R[i][0]*S[0][j] + T.R[i][1]*S[1][j]) + T.R[i][2]*S[2][j],
 *    T_s.t[i] = ((T.R[i][0]*S.t[0] + T.R[i][1]*S.t[1]) + T.R[i][2]*S.t[2]) + T.t[i].  T and T_s are then rounded to float32.  (Working
 *    in the predicted pose's object frame keeps the float32 magnitudes at the object's size instead of the camera distance.)
 *  - Per model point p_j = (x, y, z), in float32 without contraction: q_j = ((R0*x + R1*y) + R2*z) + t per row of T;
 *    d_j = sqrtf((dx*dx + dy*dy) + dz*dz) of q_j - p_j;  e_j = sqrtf(min_i |q_j - p_i|^2), the squared distance written as for d_j and
 *    computed directly (not as |q|^2 + |p|^2 - 2 q.p), the minimum over every model point i.
 *  - add = (sum_j d_j) / P, adds = (sum_j e_j) / P, add_sym = min_s (sum_j d_j(T_s)) / P, mssd = min_s max_j d_j(T_s): the sums in
 *    float64 in an order that depends on P alone (no floating-point atomics), so row n of a batch has the bits of the call on pose n
 *    alone and every replay the bits of the first run; the maximum in float32, exact.  With S_0 = I, d_j(T_0) = d_j bit for bit.
 * A relative transform T that is not finite after the rounding to float32 (a NaN or an infinity in the pose or the ground truth) gives
 * NaN in every column of that row; a T_s that is not finite gives NaN in add_sym and mssd.  Non-finite model points give unspecified
 * values.  A gt_index outside 0..G-1 reads nothing and gives NaN in every column of that row.  N == 0 does nothing.  No allocation, no host
 * synchronisation (graph-capturable); nothing is written outside out and workspace (fp_pose_errors_workspace_bytes(N, P, S) bytes,
 * 8-byte aligned; 0 for N == 0; monotone in N, P and S; it depends on S and not on flags: S symmetries without FP_ERR_SYM still have
 * their transforms formed and their room in the workspace, so pass S = 0 when the symmetric columns are not wanted).  Argument errors (FP_ERR_INVALID_ARG): NULL model_pts / poses / gt / out with
 * N > 0, P outside 1..2^22, N outside 0..65535, G < 1, S outside 0..4096, S > 0 with NULL sym_tfs, FP_ERR_SYM with S == 0, flags 0
 * or with an unknown bit, gt_index NULL when G is neither 1 nor N, a workspace that is too small or misaligned. */
size_t fp_pose_errors_workspace_bytes(int N, int P, int S);
int fp_pose_errors(const float* model_pts /*dev P,3*/, int P, const double* sym_tfs /*dev S,16|NULL*/, int S,
                   const float* poses /*dev N,16*/, const double* gt /*dev G,16*/, const int32_t* gt_index /*dev N|NULL*/, int G, int N,
                   int flags, double* out /*dev N,4*/, void* workspace /*dev*/, size_t workspace_bytes, void* stream);
/* The pixel counts of BOP's visible surface discrepancy (VSD) for N estimated poses against their ground truths, from depth renders.
 * All images share one pixel grid of h x w pixels whose top-left pixel is frame pixel (x0, y0) (full frame: x0 = y0 = 0, h x w = H x W):
 *   est (N,h,w), gt (G,h,w): rendered depth (camera z, metres, 0 = nothing rendered) at the estimated / the ground-truth poses; pose n
 *     has ground truth g = gt_index[n] (NULL: g = 0 for G == 1, g = n for G == N);
 *   obs (H,W): the raw sensor depth in metres;  fac (H,W): the depth-to-distance factor of the frame's pixels, made by the caller as
 *     fac[v][u] = float32(sqrt(1 + ((u - cx)/fx)^2 + ((v - cy)/fy)^2)) in float64 with integer u, v (BOP's depth_im_to_dist_im_fast);
 *   delta (BOP: 0.015 m); thr[T] (host), 1 <= T <= FP_VSD_MAX_T: thr[t] = float32(tau_t * diameter).
 * Per pixel, float32 without contraction, one rounding per operation (obs and fac read at the pixel's frame position):
 *   Do = obs * fac;  De = est[n] * fac;  Dg = gt[g] * fac
 *   seen = Do > 0                                            (false for 0, negatives and NaN: no measurement)
 *   vis(Dm) = Dm > 0 && (!seen || (Dm - Do) <= delta)
 *   vg = vis(Dg);  ve = vis(De) || (vg && De > 0);  inter = vg && ve;  union = vg || ve;  dist = |Dg - De|
 * counts[n] = {n_gt_vis = #vg, n_est_vis = #ve, n_inter, n_union, c_0 .. c_{T-1}} with c_t = #(inter && dist >= thr[t]), int32[4 + T].
 * On the host vsd_t = (c_t + n_union - n_inter) / n_union, and 1 for n_union == 0.  A gt_index outside 0..G-1 reads nothing and gives
 * a row of -1.  The counts are integers (integer atomics on rows the entry point clears itself on the stream): they do not depend on
 * what counts held before, a row has the same values alone and in a batch, and every replay repeats them.  Rows of 16-byte-aligned
 * groups of 4 pixels are read with 16-byte loads (w, W and x0 multiples of 4 and 16-byte-aligned pointers), anything else pixel by
 * pixel, with the same result.  N == 0 does nothing.  No allocation, no host synchronisation (graph-capturable; thr is read during the
 * call), nothing is written outside counts.  Argument errors (FP_ERR_INVALID_ARG): NULL est / gt / obs / fac / counts with N > 0, NULL
 * thr, T outside 1..FP_VSD_MAX_T, N outside 0..65535, G < 1, gt_index NULL when G is neither 1 nor N, h / w / H / W below 1, more than
 * 2^28 pixels in the window or the frame, a window that is not inside the frame, delta or a thr[t] that is negative or not finite. */
#define FP_VSD_MAX_T 16
int fp_vsd_counts(const float* est /*dev N,h,w*/, const float* gt /*dev G,h,w*/, const int32_t* gt_index /*dev N|NULL*/, int G, int N,
                  int h, int w, const float* obs /*dev H,W*/, const float* fac /*dev H,W*/, int H, int W, int x0, int y0, float delta,
                  const float* thr /*host T*/, int T, int32_t* counts /*dev N,4+T*/, void* stream);
/* BOP's maximum symmetry-aware projection distance in pixels: out[n] = min over s of max over model points p of
 * || proj(P_n p) - proj(M_s p) ||, M_s = gt_g * S_s (S == 0: M_0 = gt_g), g as in fp_pose_errors.
 *  - P_n is the float32 pose as given.  M_s is formed in float64, every 3-term sum as (a0*b0 + a1*b1) + a2*b2:
 *    M.R[i][j] = (G.R[i][0]*S.R[0][j] + G.R[i][1]*S.R[1][j]) + G.R[i][2]*S.R[2][j],
 *    M.t[i] = ((G.R[i][0]*S.t[0] + G.R[i][1]*S.t[1]) + G.R[i][2]*S.t[2]) + G.t[i], and rounded to float32 once.
 *  - Per model point p = (x, y, z) and transform (R, t), in float32 without contraction: X = ((R00*x + R01*y) + R02*z) + t0, Y and Z
 *    likewise from rows 1 and 2;  u = (fx * X) / Z + cx,  v = (fy * Y) / Z + cy (K = {fx, 0, cx, 0, fy, cy, 0, 0, 1} on the host, a
 *    non-zero skew K[1] is refused);  d = sqrtf(du*du + dv*dv) with du, dv the differences of the two projections (P_n's minus M_s's).
 *  - The maximum and the minimum are exact in float32 whatever their order; out (float64) is the float32 value widened.
 * A row is NaN if its gt_index is outside 0..G-1, if P_n or any M_s is not finite in float32, or if any transformed point of either
 * side has Z <= 0 (or NaN) under any s.  One workgroup per pose; no workspace, no atomics, no allocation, no host synchronisation
 * (graph-capturable), nothing is written outside out.  N == 0 does nothing.  Argument errors (FP_ERR_INVALID_ARG): NULL K, a non-zero
 * skew, NULL model_pts / poses / gt / out with N > 0, P outside 1..2^22, N outside 0..2^20, G < 1, S outside 0..4096, S > 0 with NULL
 * sym_tfs, gt_index NULL when G is neither 1 nor N. */
int fp_mspd(const float* model_pts /*dev P,3*/, int P, const double* sym_tfs /*dev S,16|NULL*/, int S, const float* poses /*dev N,16*/,
            const double* gt /*dev G,16*/, const int32_t* gt_index /*dev N|NULL*/, int G, int N, const float* K /*host 9*/,
            double* out /*dev N*/, void* stream);

/* The exact distance from Q points to the surface of a triangle mesh: per query point the squared distance to the nearest point of any
 * triangle, that triangle's index and that point.  Brute force over every (query, triangle) pair is the definition and the
 * implementation.  Every operation below is one float32 operation (IEEE, round to nearest even), without contraction, in the order
 * written; x - y, x * y and x / y on 3-vectors are per component;  dot(x, y) = (x0*y0 + x1*y1) + x2*y2.
 * Candidate of query p for triangle f with vertices a = pos[faces[f][0]], b = pos[faces[f][1]], c = pos[faces[f][2]]: the closest
 * point q of the closed triangle by the region walk of Ericson, Real-Time Collision Detection, 5.1.5.  The first test that holds
 * gives q (a comparison with a NaN does not hold):
 *   ab = b - a;  ac = c - a;  ap = p - a;  d1 = dot(ab, ap);  d2 = dot(ac, ap);
 *     1. d1 <= 0 && d2 <= 0:                            q = a                                         (vertex a)
 *   bp = p - b;  d3 = dot(ab, bp);  d4 = dot(ac, bp);
 *     2. d3 >= 0 && d4 <= d3:                           q = b                                         (vertex b)
 *   vc = d1*d4 - d3*d2;
 *     3. vc <= 0 && d1 >= 0 && d3 <= 0:                 v = d1 / (d1 - d3);  q = a + v * ab           (edge ab)
 *   cp = p - c;  d5 = dot(ab, cp);  d6 = dot(ac, cp);
 *     4. d6 >= 0 && d5 <= d6:                           q = c                                         (vertex c)
 *   vb = d5*d2 - d1*d6;
 *     5. vb <= 0 && d2 >= 0 && d6 <= 0:                 w = d2 / (d2 - d6);  q = a + w * ac           (edge ac)
 *   va = d3*d6 - d5*d4;  e = d4 - d3;  g = d5 - d6;
 *     6. va <= 0 && e >= 0 && g >= 0:                   w = e / (e + g);  q = b + w * (c - b)         (edge bc)
 *     7. otherwise:  denom = 1 / ((va + vb) + vc);  v = vb * denom;  w = vc * denom;  q = (a + v * ab) + w * ac    (interior)
 *   dd = dot(p - q, p - q).
 * The candidate counts only when dd <= FLT_MAX.  A triangle one of whose vertex indices is outside 0..Nv-1 has NaN vertices (nothing
 * of pos is read for it), so it never counts; neither does one with a non-finite vertex that reaches dd, nor a degenerate one whose
 * quotient is 0/0 (a degenerate triangle that an earlier vertex test answers does count: the walk is followed as written).
 * The answer for p is the candidate with the smallest (dd, f) in lexicographic order: equal distances go to the smaller face index.
 *   dist2[i] = dd,  face[i] = f,  closest[i] = q.   A query that no triangle answers (a NaN query, F == 0, every triangle skipped):
 *   dist2[i] = +inf,  face[i] = -1,  closest[i] = (0, 0, 0).
 * A minimum has no summation order, so each output has one value whatever the schedule: a query has the same bits alone, in a batch
 * and on every replay.  face and closest may be NULL (not wanted).  One query per lane; the triangles pass through LDS in tiles and the
 * grid runs over (256 queries) x (a chunk of faces), the partial minima merged with 64-bit integer atomic minima on the key
 * (bits(dd) << 32) | f in the workspace -- non-negative floats order as their bits do; there are no floating-point atomics.  An init
 * launch sets the keys, and a finish launch recomputes q for the winning face with the same arithmetic and writes the outputs.  Q * F pair
 * tests of about 80 float32 operations each: the cost is the caller's to weigh (fp_mesh_grid_point_distance below answers from a uniform grid).  Q == 0 does nothing.
 * No allocation, no host synchronisation (graph-capturable); nothing is written outside the outputs and the workspace
 * (fp_mesh_point_distance_workspace_bytes(Q) bytes = 8 * Q, 8-byte aligned; 0 for Q <= 0).  Argument errors (FP_ERR_INVALID_ARG),
 * before any launch: Q, F or Nv negative, Q or F above 2^30; NULL points / dist2 with Q > 0; NULL faces with F > 0 (and Q > 0); NULL pos
 * with Nv > 0 and F > 0 (and Q > 0); a workspace that is NULL, too small or misaligned with Q > 0. */
size_t fp_mesh_point_distance_workspace_bytes(int Q);
int fp_mesh_point_distance(const float* pos /*dev Nv,3*/, int Nv, const int32_t* faces /*dev F,3*/, int F,
                           const float* points /*dev Q,3*/, int Q,
                           float* dist2 /*dev Q*/, int32_t* face /*dev Q|NULL*/, float* closest /*dev Q,3|NULL*/,
                           void* workspace /*dev*/, size_t workspace_bytes, void* stream);

/* What R rays hit first on a triangle mesh: per ray the parameter t of the first intersection, that triangle's index, the barycentric
 * coordinates of the hit and the hit point.  Brute force over every (ray, triangle) pair is the definition and the implementation.
 * Every operation below is one float32 operation (IEEE, round to nearest even), without contraction, in the order written;
 * dot(x, y) = (x0*y0 + x1*y1) + x2*y2;  x cross y = (x1*y2 - x2*y1, x2*y0 - x0*y2, x0*y1 - x1*y0), each component one difference of
 * two products.  Ray i is o + t d with o = origins[i], d = dirs[i]; d need not be a unit vector, and t is in units of d.
 * Candidate of the ray for triangle f with vertices a, b, c read as fp_mesh_point_distance reads them (Moeller and Trumbore, Fast,
 * Minimum Storage Ray/Triangle Intersection, 1997), ab = b - a, ac = c - a:
 *   pvec = d cross ac;  det = dot(ab, pvec);  tvec = o - a;  un = dot(tvec, pvec);
 *   qvec = tvec cross ab;  vn = dot(d, qvec);  tn = dot(ac, qvec);
 *   s = det < 0 ? -1 : +1;  D = |det|;  U = s*un;  V = s*vn;  T = s*tn   (exact sign changes);   t = T / D
 *   hit  <=>  D > 0  &&  U >= 0  &&  V >= 0  &&  (U + V) <= D  &&  t_min <= t <= t_max  &&  t <= FLT_MAX
 * cull: 0 keeps both sides of a face, 1 only det > 0 (the ray meets the face against its normal ab cross ac: back faces are
 * dropped), 2 only det < 0.  There is no epsilon anywhere: a degenerate triangle and a ray in a triangle's plane have det == 0 and
 * never answer; a comparison with a NaN does not hold, so a NaN or infinite vertex that reaches a test, an index outside 0..Nv-1 (NaN
 * vertices; nothing of pos is read for it), a non-finite ray and a zero direction never answer either.  The t of a hit that compares
 * equal to 0 is recorded as +0.
 * The answer of a ray is the candidate with the smallest (t, f) in lexicographic order: equal t go to the smaller face index.
 *   t[i] = t,  face[i] = f,  bary[i] = (U / D, V / D),  hit[i] = (o.x + t*d.x, o.y + t*d.y, o.z + t*d.z)
 * (the hit is a + bary.u * ab + bary.v * ac up to rounding).  A ray that nothing answers: t[i] = +inf, face[i] = -1, bary and hit NaN.
 * The intersection is NOT watertight: each triangle is tested with its own roundings, so a ray through an edge or a vertex that two
 * faces share can miss both, and where it hits both with equal t the smaller face answers.  Callers that need "is the segment
 * blocked" keep the segment's end out of the range (t_max < 1) and so do not depend on the end's own face.
 * A minimum has no summation order, so each output has one value whatever the schedule: a ray has the same bits alone, in a batch and
 * on every replay.  face, bary and hit may be NULL (not wanted).  One ray per lane; the triangles pass through the LDS tile of
 * fp_mesh_point_distance, whose a, b - a and c - a are the operands above, and the grid runs over (256 rays) x (a chunk of faces), the
 * partial minima merged with 64-bit integer atomic minima on the key (bits(t) << 32) | f in the workspace.  An init launch sets the
 * keys, and a finish launch recomputes U, V, D for the winning face with the same arithmetic and writes the outputs.  R * F pair tests;
 * R == 0 does nothing.  No allocation, no host synchronisation (graph-capturable); nothing is written outside the outputs and the
 * workspace (fp_mesh_ray_cast_workspace_bytes(R) bytes = 8 * R, 8-byte aligned; 0 for R <= 0).  Argument errors
 * (FP_ERR_INVALID_ARG), before any launch, in this order: R, F or Nv negative, R or F above 2^30; not 0 <= t_min <= t_max (t_max may
 * be +inf; a NaN is refused); cull outside 0..2; then with R > 0: NULL origins, dirs or t; NULL faces with F > 0; NULL pos with Nv > 0
 * and F > 0; a workspace that is NULL, too small or misaligned. */
size_t fp_mesh_ray_cast_workspace_bytes(int R);
int fp_mesh_ray_cast(const float* pos /*dev Nv,3*/, int Nv, const int32_t* faces /*dev F,3*/, int F,
                     const float* origins /*dev R,3*/, const float* dirs /*dev R,3*/, int R,
                     float t_min, float t_max, int cull /*0 none, 1 back faces, 2 front faces*/,
                     float* t /*dev R*/, int32_t* face /*dev R|NULL*/, float* bary /*dev R,2|NULL*/, float* hit /*dev R,3|NULL*/,
                     void* workspace /*dev*/, size_t workspace_bytes, void* stream);

/* How far does each of T candidate transforms move a mesh's surface off itself: the squared distances of Q transformed points (surface
 * samples, as a rule) to the surface, reduced per transform on the chip.  Every operation is one float32 operation (IEEE, round to
 * nearest even), without contraction, in the order written.
 *  - Transformed point.  For transform t with rows r0, r1, r2 of tfs[t] (row-major 4x4; row 3 is never read) and point i = (x, y, z):
 *      p'[k] = ((rk[0]*x + rk[1]*y) + rk[2]*z) + rk[3],  k = 0, 1, 2.
 *    The rows are used as given: a matrix that is no rigid motion is not an error.
 *  - Distance.  d2(t, i) is dist2 of fp_mesh_point_distance for the query p': the smallest dd over the triangles whose candidate
 *    counts (dd <= FLT_MAX), by exactly that function's closest-point walk (one copy of the code, csrc/mesh_closest.h), and +inf
 *    where no triangle answers: F == 0, every triangle skipped, or a p' that is not finite.  d2 is never NaN and never negative.
 *  - Outputs.  max_d2[t] = the maximum over i of d2(t, i) (+inf if any sample is unanswered);  over[t*L + l] = the number of i with
 *    d2(t, i) > thr2[l], strictly, so +inf counts unless thr2[l] is +inf, and a NaN threshold counts nothing;  dist2[t*Q + i] =
 *    d2(t, i), where asked for.  over may be NULL when L == 0, dist2 may be NULL (not wanted).
 *  - Empty inputs.  T == 0 does nothing.  With Q == 0 (and T > 0) max_d2[t] = 0 and over[t, l] = 0; dist2 has no element.
 * Every reduction is a minimum, a maximum or an integer count, the first two taken on the bits of non-negative floats (which order as
 * the floats do), so each output has one value whatever the schedule: a transform has the same bits alone, in a batch and on every
 * replay.  Integer atomics only.  The grid runs over (256 (transform, sample) pairs, numbered t*Q + i, one per lane) x (a chunk of
 * faces); the triangles pass through LDS in tiles; a lane merges its chunk's minimum into workspace[t*Q + i] with one 32-bit atomic
 * minimum; an init launch sets the cells to the bits of +inf and a finish launch, one workgroup per transform, takes the maximum and
 * the counts.  T * Q * F pair tests: the cost is the caller's to weigh.  No allocation, no host synchronisation (graph-capturable);
 * nothing is written outside the outputs and the workspace (fp_mesh_transform_residuals_workspace_bytes(T, Q) bytes = 4 * T * Q,
 * 4-byte aligned; 0 when T <= 0 or Q <= 0).  Argument errors (FP_ERR_INVALID_ARG), before any launch, each message beginning with
 * the entry point's name: T, Q, F or Nv negative; T * Q, T or F above 2^30; L outside 0..4; and with T > 0: NULL max_d2; NULL thr2 or
 * over with L > 0; with Q > 0 also NULL points or tfs, NULL faces with F > 0, NULL pos with Nv > 0 and F > 0, a workspace that is
 * NULL, too small or misaligned. */
size_t fp_mesh_transform_residuals_workspace_bytes(int T, int Q);
int fp_mesh_transform_residuals(const float* pos /*dev Nv,3*/, int Nv, const int32_t* faces /*dev F,3*/, int F,
                                const float* points /*dev Q,3*/, int Q,
                                const float* tfs /*dev T,4,4 row-major; rows 0..2 are read*/, int T,
                                const float* thr2 /*dev L | NULL when L == 0*/, int L /*0..4*/,
                                float* max_d2 /*dev T*/, int32_t* over /*dev T,L|NULL*/, float* dist2 /*dev T,Q|NULL*/,
                                void* workspace /*dev*/, size_t workspace_bytes, void* stream);

/* Register one mesh onto another: ONE Gauss-Newton step of point-to-plane ICP for each of T candidate transforms of Q points (surface
 * samples of a mesh a) against the surface of a triangle mesh b (pos, faces), in four launches.  Defined to the operation.
 * Per pair (t, i), float32, one rounding per operation, without contraction, every 3-term sum as (a0*b0 + a1*b1) + a2*b2:
 *   p = the point as fp_mesh_transform_residuals forms it: p[k] = ((rk[0]*x + rk[1]*y) + rk[2]*z) + rk[3] per row rk of tfs_in[t];
 *       row 3 is not read;
 *   (dd, f, q) = exactly fp_mesh_point_distance's dist2, face and closest for the query p: the smallest (dd, face) wins, by that
 *       function's closest-point walk (one copy of the code, csrc/mesh_closest.h); (+inf, -1, -) where no triangle answers;
 *   the normal of face f with ab = b - a, ac = c - a:  n = ab x ac = (ab1*ac2 - ab2*ac1, ab2*ac0 - ab0*ac2, ab0*ac1 - ab1*ac0) in
 *       float32;  nn = (n0*n0 + n1*n1) + n2*n2 in float64 of the widened components;  m_k = (float)((double)n_k / sqrt(nn)) (the
 *       float64 division and square root are correctly rounded);
 *   e = q - p;   r = m.e;   a = p - c with c = (tfs_in[t][3], [7], [11]);
 *   J = (a1*m2 - a2*m1, a2*m0 - a0*m2, a0*m1 - a1*m0, m0, m1, m2): the convention of fp_icp_point_plane, the step rotates about the
 *       transform's own origin, p' = c + dR(w) (p - c) + v;
 *   pair = f >= 0 && nn > 0 && m0, m1, m2 finite && dd <= max_dist * max_dist (the product in float32; it may be +inf).  A NaN
 *       anywhere makes it no pair.
 * dist2[t*Q + i] = dd and face[t*Q + i] = f, where asked for, are written for every (t, i), pair or not.
 * Per transform, float64: the 28 sums of fp_icp_point_plane (A = sum J^T J, its 21 upper entries; b = sum J^T r; sum r*r), the pair
 * count, and the sum of dd over the pairs (each dd widened), every term exact.  The sums run over chunks of 256 consecutive samples,
 * inside a chunk over 4 waves of 64: within a wave by the xor tree (s += s of lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; a sample that is no
 * pair adds +0), the waves in index order, then the chunks in index order starting from +0 (one copy of the code with
 * fp_icp_point_plane, csrc/icp_solve.h).  The order depends on Q alone and there are no floating-point atomics (the nearest face is
 * merged with 64-bit integer atomic minima on (bits(dd) << 32) | f): row t has the same bits alone, in any batch, in any order of
 * tfs_in, under any chunking of the faces and on every replay.
 * Solve, status and update exactly as fp_icp_point_plane defines them, with tfs_in in the place of poses_in: damping on diag(A), LDL^T
 * without pivoting, status 0 solved / 1 fewer than min_pairs pairs / 2 a non-finite tfs_in row (all 16), a pivot <= 0 or not finite
 * or a non-finite x; Rodrigues in float64, R' = dR * R_in, t' = t_in + v, each rounded once to float32, row 3 copied; for status != 0,
 * x = 0 and the tfs_out row is the tfs_in row bit for bit.
 * system[t] (float64 x 40): fp_icp_point_plane's layout, [0..20] A's upper triangle row-major, [21..26] b, [27] sum r*r, [28] pairs,
 * [29] status, [30..35] x, and [36] the sum of dd over the pairs, [37..39] 0.  The sums are reported whatever the status.
 * tfs_out, dist2 and face may be NULL (not wanted); tfs_in and tfs_out must not overlap.  T == 0 does nothing.  Q == 0 or F == 0 gives
 * zero sums and no pair (status 1, or 2 for a non-finite row) and tfs_out = tfs_in; with F == 0, dist2 = +inf and face = -1.
 * T * Q * F pair tests: the cost is the caller's to weigh.  No allocation, no memset, no host synchronisation (graph-capturable);
 * nothing is written outside the outputs and the workspace (fp_mesh_icp_workspace_bytes(T, Q) bytes = 8 * T * Q for the keys and 256
 * per (transform, chunk of 256 samples), 8-byte aligned; 0 when T <= 0 or Q <= 0).  Argument errors (FP_ERR_INVALID_ARG), before
 * any launch, each message beginning with the entry point's name: T, Q, F or Nv negative; T * Q, T or F above 2^30; max_dist or
 * damping negative or not finite; min_pairs < 6; and with T > 0: NULL tfs_in or system; with Q > 0 also NULL points, NULL faces with
 * F > 0, NULL pos with Nv > 0 and F > 0, a workspace that is NULL, too small or misaligned; tfs_in overlapping tfs_out. */
size_t fp_mesh_icp_workspace_bytes(int T, int Q);
int fp_mesh_icp_step(const float* pos /*dev Nv,3*/, int Nv, const int32_t* faces /*dev F,3*/, int F,
                     const float* points /*dev Q,3*/, int Q,
                     const float* tfs_in /*dev T,4,4 row-major*/, int T, float max_dist, double damping, int min_pairs,
                     double* system /*dev T,40*/, float* tfs_out /*dev T,16|NULL*/,
                     float* dist2 /*dev T,Q|NULL*/, int32_t* face /*dev T,Q|NULL*/,
                     void* workspace /*dev*/, size_t workspace_bytes, void* stream);

/* Which side of a closed mesh: the angle-weighted pseudonormals of its vertices and edges (Baerentzen and Aanaes, Signed distance
 * computation using the angle weighted pseudonormal, 2005), and a report of what keeps the mesh from being closed.  HOST pointers, no
 * device, setup time (as fp_cluster_poses).  Every operation is float64 on the widened float32 coordinates, each output rounded once
 * to float32; acos is the host libm's.
 *  - Welding.  Adjacency goes by position, not by index (OBJ files repeat a vertex along UV seams): two indices whose three float32
 *    coordinates compare equal (-0 == +0; a NaN equals nothing, itself included) are one vertex, named w(i) = the smallest such index.
 *  - Faces.  Face f with a, b, c = pos[faces[f][0..2]]:  n = (b - a) x (c - a), len = sqrt((n0*n0 + n1*n1) + n2*n2), u_f = n / len.
 *    The face is DEGENERATE when an index is outside 0..Nv-1 or len is not a finite number above 0; a degenerate face has no normal
 *    and takes no part in anything below.
 *  - vn[i] = the sum, over the non-degenerate faces f in index order and their corners j = 0, 1, 2 in order with w(faces[f][j]) = w(i),
 *    of angle * u_f, where angle = acos(clamp(dot(e0, e1) / (|e0| * |e1|), -1, 1)) for the edges e0, e1 from corner j to the next and
 *    to the previous corner.  Not normalised: only its direction is used.  An index that no such face uses has vn = 0.
 *  - en[f][k], k = 0, 1, 2 for the edges ab, bc, ca of face f = the sum of u_g over the non-degenerate faces g, in index order, that have
 *    an edge with the same unordered pair of welded end points.  For a face with an index outside the table it is 0; for any other
 *    degenerate face it is that same sum (0 when no non-degenerate face has the edge).  A boundary edge carries its one face's normal.
 *  - report[0] the distinct edges (unordered welded pairs) of the non-degenerate faces; [1] those with one face (boundary); [2] those
 *    with more than two faces (non-manifold); [3] those with exactly two faces that both traverse it in the same direction
 *    (inconsistently oriented); [4] the degenerate faces; [5] the indices i with w(i) != i (welded away); [6] closed: 1 when [0] > 0 and
 *    [1] = [2] = [3] = 0, else 0; [7] 0.
 * For a closed, consistently outward-oriented mesh that does not intersect itself, the sign of (p - q) . n with q the closest point of
 * the surface to p and n the pseudonormal of the feature q lies on (vn at a vertex, en on an edge, u_f in a face) is negative exactly
 * for p inside.  The report cannot see self-intersection, several shells or an inward orientation: those are the caller's to exclude.
 * Argument errors (FP_ERR_INVALID_ARG): Nv or F outside 0..2^30, NULL report, NULL pos / vn with Nv > 0, NULL faces / en with F > 0. */
int fp_mesh_pseudonormals(const float* pos /*host Nv,3*/, int Nv, const int32_t* faces /*host F,3*/, int F,
                          float* vn /*host Nv,3*/, float* en /*host F,3,3*/, int32_t* report /*host 8*/);

/* The signed distance from Q points to a mesh: fp_mesh_point_distance and the side.  dist2, face and closest are that function's, by
 * the same launches on the same code (csrc/mesh_closest.h): the same bits for the same inputs.  vn and en are fp_mesh_pseudonormals'
 * tables on the device.  For a query p that a triangle answers, with f its face, q its closest point and a, b, c, ab, ac as above:
 *   feature[i] = where the walk found q: 0, 1, 2 vertex a, b, c (tests 1, 2, 4); 3, 4, 5 edge ab, bc, ca (tests 3, 6, 5); 6 interior (7);
 *   n = vn[faces[f][feature]] for a vertex;  en[f][feature - 3] for an edge;  for the interior ab x ac in float32 =
 *       (ab1*ac2 - ab2*ac1, ab2*ac0 - ab0*ac2, ab0*ac1 - ab1*ac0), each component one difference of two products;
 *   s = dot(p - q, n) (float32, dot as above);  sign[i] = -1 when s < 0, else +1.
 * So s = 0 (a point on the surface, a zero n), a NaN s and s > 0 are all outside.  The signed distance is sign * sqrt(dist2).
 * A query that no triangle answers: dist2 = +inf, face = -1, closest = 0, feature = -1, sign = 0.
 * face, closest, feature and sign may each be NULL (not wanted).  Three launches (init, scan, finish: the finish walks the winning face
 * again); no allocation, no host synchronisation (graph-capturable); nothing is written outside the outputs and the workspace
 * (fp_mesh_signed_distance_workspace_bytes(Q) bytes = 8 * Q, 8-byte aligned; 0 for Q <= 0).  Q == 0 does nothing.  Argument errors
 * (FP_ERR_INVALID_ARG), before any launch, each message beginning with the entry point's name: fp_mesh_point_distance's, and with
 * Q > 0 and F > 0 a NULL en, or a NULL vn with Nv > 0. */
size_t fp_mesh_signed_distance_workspace_bytes(int Q);
int fp_mesh_signed_distance(const float* pos /*dev Nv,3*/, int Nv, const int32_t* faces /*dev F,3*/, int F,
                            const float* vn /*dev Nv,3*/, const float* en /*dev F,3,3*/, const float* points /*dev Q,3*/, int Q,
                            float* dist2 /*dev Q*/, int32_t* face /*dev Q|NULL*/, float* closest /*dev Q,3|NULL*/,
                            int32_t* feature /*dev Q|NULL*/, int32_t* sign /*dev Q|NULL*/,
                            void* workspace /*dev*/, size_t workspace_bytes, void* stream);

/* How far each of T placements of Q points reaches into a mesh.  The point of pair (t, i) is p' exactly as
 * fp_mesh_transform_residuals forms it (rows 0..2 of tfs[t] as given, row 3 never read); (dd, sign) are fp_mesh_signed_distance's dist2
 * and sign for the query p'.  Per transform t:
 *   inside[t]  = the number of i with sign = -1;
 *   depth2[t]  = the largest dd among them, 0 when there are none;
 *   deepest[t] = the i of that dd, the smallest i among equal dd, -1 when there are none;
 *   sign[t*Q + i], dist2[t*Q + i] = the pair's values, where asked for.
 * A row 0..2 of tfs[t] with a non-finite element (or a product that overflows) makes p' non-finite, no triangle answers it, and so:
 * sign = 0, dist2 = +inf, and a transform all of whose p' are such has inside = 0, depth2 = 0, deepest = -1.  The same holds with
 * Q == 0 or F == 0.  T == 0 does nothing.  depth2, deepest, sign and dist2 may each be NULL (not wanted).
 * The count is an integer sum and the deepest point a 64-bit integer maximum of (bits(dd) << 32) | ~i, both by LDS atomics in one
 * workgroup per transform; the nearest face is merged with 64-bit integer atomic minima as in fp_mesh_point_distance: every output has
 * one value whatever the schedule, and row t has the same bits alone, in any batch and on every replay.  Three launches; T * Q * F pair
 * tests.  No allocation, no memset, no host synchronisation (graph-capturable); nothing is written outside the outputs and the
 * workspace (fp_mesh_penetration_workspace_bytes(T, Q) bytes = 8 * T * Q, 8-byte aligned; 0 when T <= 0 or Q <= 0).  Argument errors
 * (FP_ERR_INVALID_ARG), before any launch, each message beginning with the entry point's name: T, Q, F or Nv negative; T * Q, T or F
 * above 2^30; and with T > 0: NULL inside; with Q > 0 also NULL points or tfs, NULL faces or en with F > 0, NULL pos or vn with Nv > 0
 * and F > 0, a workspace that is NULL, too small or misaligned. */
size_t fp_mesh_penetration_workspace_bytes(int T, int Q);
int fp_mesh_penetration(const float* pos /*dev Nv,3*/, int Nv, const int32_t* faces /*dev F,3*/, int F,
                        const float* vn /*dev Nv,3*/, const float* en /*dev F,3,3*/, const float* points /*dev Q,3*/, int Q,
                        const float* tfs /*dev T,4,4 row-major; rows 0..2 are read*/, int T,
                        int32_t* inside /*dev T*/, float* depth2 /*dev T|NULL*/, int32_t* deepest /*dev T|NULL*/,
                        int32_t* sign /*dev T,Q|NULL*/, float* dist2 /*dev T,Q|NULL*/,
                        void* workspace /*dev*/, size_t workspace_bytes, void* stream);

/* A uniform grid over a mesh's triangles, and fp_mesh_point_distance / fp_mesh_signed_distance answered from it: the same outputs, bit
 * for bit, from a few dozen pair tests a query near the surface instead of F.  The answer is a minimum over (dd, f) keys, which
 * commutes: which triangles are skipped never shows in a result as long as no skipped triangle could have won or tied, and the stop rule
 * below is proved to skip only such triangles under one precondition on the float32 closest points (stated at the end).
 *
 * The grid (fp_mesh_grid, a host struct): an origin lo[3], a cell edge h, n[3] cells, a slack pad; all float32 / int32, chosen by the
 * caller.  inv_h = 1.f / h.  M = max_k max(|lo_k|, |lo_k + float(n_k) * h|).  Refused (FP_ERR_INVALID_ARG): a non-finite lo, h or pad;
 * h outside 2^-100..2^100 (so h <= 0 too); an n_k < 1; more than 2^21 cells; a non-finite M; pad < 2^-20 * M.
 *   cell_k(x) = (int)clamp(floorf((x - lo_k) * inv_h), 0, n_k - 1), clamped in float before the conversion; cell (ix, iy, iz) has the
 *   linear index (iz * n_1 + iy) * n_0 + ix.
 * A triangle f, its vertices read as fp_mesh_point_distance reads them, is
 *   dropped   when an index is outside 0..Nv-1 (it never counts in the brute force either);
 *   overflow  when its indices are valid and a vertex coordinate is not finite, or its cell range below covers more than 4096 cells:
 *             every query tests every triangle of this list (a triangle with an infinite vertex can give a finite dd);
 *   stored    otherwise, in every cell of cell_k(tmin_k - pad) .. cell_k(tmax_k + pad) on each axis k (tmin, tmax its bounding box; the
 *             clamp puts a triangle outside the grid's box into boundary cells).
 * fp_mesh_grid_count zeroes cell_start, adds 1 to every cell of a stored triangle's range, takes the exclusive scan into
 * cell_start[ncells + 1] and writes header[4] = {n_entries (= cell_start[ncells]), n_overflow, status, 0} on the device.
 * fp_mesh_grid_fill, given that cell_start, entries[grid->n_entries] and overflow[grid->n_overflow] (the capacities) and a cursor
 * workspace of (ncells + 1) int32, writes each stored triangle's index into a slot of each of its cells (an atomic cursor per cell: the
 * order inside a cell is arbitrary and shows in no result) and the overflow list, by the same per-triangle decision (one device
 * function).  It writes nothing past a capacity or past a cell's own slots: if one was too small it ORs FP_MESH_GRID_ENTRIES_TOO_SMALL
 * / FP_MESH_GRID_OVERFLOW_TOO_SMALL into header[2] (count sets it to 0, or to FP_MESH_GRID_TOO_MANY_ENTRIES when the lists would hold
 * more than 2^31 - 1 entries).  Both run on the caller's stream with integer atomics only, allocate nothing and do not synchronise;
 * the caller reads the header between them to size the lists.
 *
 * The walk of a query p.  A non-finite p answers nothing (p - q has an infinite or NaN component for every q, so no dd counts) and
 * walks nothing.  Otherwise c_k = cell_k(p_k), and for r = 0, 1, 2, ... the cells at Chebyshev distance r from c that are in the grid
 * are visited; every entry f of a visited cell is tested -- dd exactly as above, on a, b, c, b - a, c - a -- and replaces the best
 * when dd < best || (dd == best && f < best_f).  After shell r, for each axis k:
 *   high side, when c_k + r < n_k - 1:  X = lo_k + (float)(c_k + r + 1) * h;  m_k+ = X - p_k
 *   low side,  when c_k - r > 0:        X = lo_k + (float)(c_k - r) * h;      m_k- = p_k - X
 * and m = the smallest of those that exist.  The walk stops when none exists (the block is the whole grid) or when m > 0 and
 * best < m * m (strictly; one float32 product).  Then every triangle of the overflow list is tested the same way.
 *
 * Why no skipped triangle wins or ties (u = 2^-24; the high side of axis k, the low side mirrors it).  A stored triangle outside the
 * block has, on some axis, i0 = cell_k(s) >= j = c_k + r + 1 with s = fl(tmin_k - pad), and j <= n_k - 1, so the clamp did not raise
 * it: fl(fl(s - lo_k) * inv_h) >= j.  Three roundings (the difference, inv_h, the product) give s - lo_k >= j*h*(1 - 3u), and
 * j*h <= 2M, so s >= (lo_k + j*h) - 6uM.  X = fl(lo_k + fl(j*h)) has two roundings, of a product <= 2M and of a sum <= M:
 * X <= (lo_k + j*h) + 3uM.  s itself is one rounding of tmin_k - pad, at most 2uM when |tmin_k - pad| <= 2M (beyond 2M the triangle is
 * farther than M past X and the claim is immediate).  Together tmin_k >= X + pad - 11uM(1 + O(u)).  With the precondition
 * q_k >= tmin_k - pad / 4 and pad >= 2^-20 * M = 16uM:  q_k >= X + (12 - 11)uM > X, both float32 numbers, so by the monotonicity of
 * rounding fl(q_k - p_k) >= fl(X - p_k) = m > 0.  In dd = dot(p - q, p - q) the component's square is then >= fl(m * m), every other
 * term is >= 0 and adding a non-negative term never lowers a rounded sum: dd >= fl(m * m) > best.  Triangles clamped into boundary
 * cells are covered because a side whose block touches the grid's end contributes no plane.
 * THE PRECONDITION: for every (query, triangle) pair with dd <= FLT_MAX, the computed q lies within pad / 4 of the triangle's bounding
 * box on each axis.  Under it, dist2, face, closest (and feature, sign) equal the brute-force entry points' bit for bit.  The walk's q
 * is a vertex or a + s*dir (+ w*ac) with s, w in [0, 1] up to rounding, so it leaves the box by a few u of the triangle's largest
 * coordinate (1.43 * 2^-24 of it is the largest measured over the generated cases); pad = 2^-16 * M, the default of the Python
 * wrapper, allows 2^-18 * M = 64 u M, some 45 times that.  tests/test_mesh_grid_host.py checks the precondition for every case and grid it uses.
 *
 * fp_mesh_grid_point_distance and fp_mesh_grid_signed_distance: the parents' init launch, a scan of 256 queries a workgroup, one per
 * lane, that walks as above and merges into the same 64-bit key, and the parents' finish kernels unchanged -- the keys workspace is the
 * interface, so every output is made by the code that makes it today.  The workspace is the parent's (8 * Q bytes).  No allocation, no
 * host synchronisation (graph-capturable).  grid->n_entries and grid->n_overflow are the lengths of the lists here; an entry outside
 * 0..F-1 is ignored, and nothing outside the tables' lengths is read.  Argument errors: the parent's, each message beginning with the
 * entry point's name, and the grid's refusals above, a NULL grid, a NULL cell_start, NULL entries / overflow with a length > 0, a
 * negative length; for count and fill also a NULL header, and for fill a NULL or misaligned cursor workspace.
 *
 * fp_mesh_grid_transform_residuals, fp_mesh_grid_icp_step and fp_mesh_grid_penetration: fp_mesh_transform_residuals, fp_mesh_icp_step
 * and fp_mesh_penetration with the grid after F, each to its parent what fp_mesh_grid_point_distance is to fp_mesh_point_distance.  The
 * parent's init launch; a scan of 256 (transform, sample) pairs a workgroup, numbered t*Q + i, one per lane, in which the lane forms
 * p' = ((rk[0]*x + rk[1]*y) + rk[2]*z) + rk[3] exactly as the parent does and walks as above for the query p', merging into the
 * parent's cell (the 32-bit bits(dd) of the residuals, the 64-bit key of the other two); then the parent's finish kernels unchanged.
 * The proof of the stop rule above is per query point: it uses p only as a float32 point whose cell and plane distances the walk
 * computes from it, so it holds unchanged for p', however p' was formed, and a non-finite p' walks nothing and answers nothing, as in
 * the brute force.  Every output -- max_d2, over, dist2; system with its float64 sums, tfs_out, dist2, face; inside, depth2, deepest,
 * sign, dist2 -- has the parent's bits under the precondition above.  The workspace is the parent's, sized by the parent's
 * *_workspace_bytes function.  No allocation, no memset, no host synchronisation (graph-capturable), integer atomics only.  The cost
 * is per pair: a p' within about a cell of the surface tests a few dozen triangles; a p' a few cells away tests hundreds, each a gather
 * from global memory that only its lane wants, and is already slower than the brute force's LDS tiles; a p' far from the mesh walks
 * shell after shell until the whole grid is visited and tests every stored triangle -- the grid form is for samples near the surface.
 * Argument errors, before any launch, each message beginning with the new entry point's name: the parent's, and, after the parent's
 * checks of T, Q, F and Nv, the grid's refusals as listed above. */
typedef struct fp_mesh_grid {
  float lo[3];
  float h;
  int32_t n[3];
  float pad;
  int32_t* cell_start;   /* dev ncells + 1 */
  int32_t* entries;      /* dev n_entries | NULL when 0 */
  int32_t* overflow;     /* dev n_overflow | NULL when 0 */
  int32_t n_entries;     /* fill: the capacity of entries; queries: its length */
  int32_t n_overflow;    /* fill: the capacity of overflow; queries: its length */
} fp_mesh_grid;
#define FP_MESH_GRID_ENTRIES_TOO_SMALL 1
#define FP_MESH_GRID_OVERFLOW_TOO_SMALL 2
#define FP_MESH_GRID_TOO_MANY_ENTRIES 4
#define FP_MESH_GRID_MAX_CELLS (1 << 21)
#define FP_MESH_GRID_MAX_CELLS_PER_TRIANGLE 4096
int fp_mesh_grid_count(const float* pos /*dev Nv,3*/, int Nv, const int32_t* faces /*dev F,3*/, int F,
                       const fp_mesh_grid* grid /*host; cell_start is written, the lists are not read*/,
                       int32_t* header /*dev 4*/, void* stream);
size_t fp_mesh_grid_fill_workspace_bytes(const fp_mesh_grid* grid /*host*/);   /* 4 * (ncells + 1); 0 for a grid that is refused */
int fp_mesh_grid_fill(const float* pos /*dev Nv,3*/, int Nv, const int32_t* faces /*dev F,3*/, int F,
                      const fp_mesh_grid* grid /*host; entries and overflow are written*/,
                      int32_t* header /*dev 4, as count left it*/, void* workspace /*dev*/, size_t workspace_bytes, void* stream);
int fp_mesh_grid_point_distance(const float* pos /*dev Nv,3*/, int Nv, const int32_t* faces /*dev F,3*/, int F,
                                const fp_mesh_grid* grid /*host*/, const float* points /*dev Q,3*/, int Q,
                                float* dist2 /*dev Q*/, int32_t* face /*dev Q|NULL*/, float* closest /*dev Q,3|NULL*/,
                                void* workspace /*dev*/, size_t workspace_bytes, void* stream);
int fp_mesh_grid_signed_distance(const float* pos /*dev Nv,3*/, int Nv, const int32_t* faces /*dev F,3*/, int F,
                                 const fp_mesh_grid* grid /*host*/, const float* vn /*dev Nv,3*/, const float* en /*dev F,3,3*/,
                                 const float* points /*dev Q,3*/, int Q,
                                 float* dist2 /*dev Q*/, int32_t* face /*dev Q|NULL*/, float* closest /*dev Q,3|NULL*/,
                                 int32_t* feature /*dev Q|NULL*/, int32_t* sign /*dev Q|NULL*/,
                                 void* workspace /*dev*/, size_t workspace_bytes, void* stream);
int fp_mesh_grid_transform_residuals(const float* pos /*dev Nv,3*/, int Nv, const int32_t* faces /*dev F,3*/, int F,
                                     const fp_mesh_grid* grid /*host*/, const float* points /*dev Q,3*/, int Q,
                                     const float* tfs /*dev T,4,4 row-major; rows 0..2 are read*/, int T,
                                     const float* thr2 /*dev L | NULL when L == 0*/, int L /*0..4*/,
                                     float* max_d2 /*dev T*/, int32_t* over /*dev T,L|NULL*/, float* dist2 /*dev T,Q|NULL*/,
                                     void* workspace /*dev*/, size_t workspace_bytes, void* stream);
int fp_mesh_grid_icp_step(const float* pos /*dev Nv,3*/, int Nv, const int32_t* faces /*dev F,3*/, int F,
                          const fp_mesh_grid* grid /*host*/, const float* points /*dev Q,3*/, int Q,
                          const float* tfs_in /*dev T,4,4 row-major*/, int T, float max_dist, double damping, int min_pairs,
                          double* system /*dev T,40*/, float* tfs_out /*dev T,16|NULL*/,
                          float* dist2 /*dev T,Q|NULL*/, int32_t* face /*dev T,Q|NULL*/,
                          void* workspace /*dev*/, size_t workspace_bytes, void* stream);
int fp_mesh_grid_penetration(const float* pos /*dev Nv,3*/, int Nv, const int32_t* faces /*dev F,3*/, int F,
                             const fp_mesh_grid* grid /*host*/, const float* vn /*dev Nv,3*/, const float* en /*dev F,3,3*/,
                             const float* points /*dev Q,3*/, int Q,
                             const float* tfs /*dev T,4,4 row-major; rows 0..2 are read*/, int T,
                             int32_t* inside /*dev T*/, float* depth2 /*dev T|NULL*/, int32_t* deepest /*dev T|NULL*/,
                             int32_t* sign /*dev T,Q|NULL*/, float* dist2 /*dev T,Q|NULL*/,
                             void* workspace /*dev*/, size_t workspace_bytes, void* stream);

/* An object's mesh from posed RGB-D reference views: truncated-signed-distance (TSDF) fusion into a caller-owned volume, then marching
 * tetrahedra.  The volume has nz x ny x nx voxels; voxel (ix, iy, iz) has the linear index i = (iz * ny + iy) * nx + ix and, in the
 * object frame, the position p = (ox + float(ix) * s, oy + float(iy) * s, oz + float(iz) * s) (origin o = {ox, oy, oz} and pitch s in
 * metres; every operation below is float32 without contraction, one rounding per operation, in the order written).  Its arrays:
 * tsdf (nz,ny,nx) in units of trunc, 1 where never observed; weight (nz,ny,nx), the number of observations; color (nz,ny,nx,3) in the
 * units of rgb; color_weight (nz,ny,nx).  A fresh volume is tsdf = 1 and zeros elsewhere (the caller fills it).
 *
 * fp_tsdf_integrate fuses V views into the volume: depth (V,H,W) metres, rgb (V,H,W,3), masks (V,H,W) uint8 (NULL: every pixel is the
 * object's), ob_in_cams (V,16) row-major object-to-camera transforms T, Ks (V,9) float64 on the device (as the crop stage's view
 * tables), rounded to float32 {fx, skew, cx, 0, fy, cy, ...}.  One voxel per lane; the views are visited inside the kernel in index
 * order, so a voxel's running means have one summation order: no atomics, every call repeats its bits, and a call over views 0..k
 * followed by a call over k+1..V-1 leaves the bits of one call over 0..V-1.  A view whose 16 pose values, fx, fy, cx, cy are not all
 * finite, or whose skew is not 0, is skipped for every voxel.  Otherwise, per voxel:
 *   X = ((T00*px + T01*py) + T02*pz) + T03, Y and Z likewise from rows 1 and 2;   skip the view unless Z > 0;
 *   u = floorf(((fx * X) / Z + cx) + 0.5f),  v = floorf(((fy * Y) / Z + cy) + 0.5f);   skip the view unless 0 <= u < W and 0 <= v < H
 *     (compared as floats: a NaN or an infinity skips);
 *   mask[v][u] == 0: the pixel saw past the object, the voxel is empty: obs = 1, no colour (this is the space carving that removes
 *     the background and the table; the views are assumed to show the object unoccluded);
 *   otherwise d = depth[v][u];  skip the view unless d >= min_depth (holes, negatives, NaN);  sdf = d - Z;  skip the view if
 *     sdf < -trunc (the voxel is hidden behind the surface);  q = sdf / trunc;  obs = q < 1 ? q : 1;
 *   tsdf = (tsdf * weight + obs) / (weight + 1);  weight = weight + 1;
 *   and, when the mask is not 0 and |sdf| <= trunc, per channel color = (color * color_weight + rgb[v][u]) / (color_weight + 1), then
 *     color_weight = color_weight + 1.
 * No index outside the frames or the volume is formed.  V == 0 does nothing.  No allocation, no host synchronisation
 * (graph-capturable; origin is read during the call); nothing is written outside the four arrays.
 *
 * fp_tsdf_count_triangles: counts[c] (int32, 0..12) for each of the (nz-1)(ny-1)(nx-1) cubes, c = (cz * (ny-1) + cy) * (nx-1) + cx,
 * whose corner of smallest index is voxel (cx, cy, cz).  A cube is split along its main diagonal into the six Kuhn tetrahedra, one per
 * permutation (a, b, c) of the axes (x = 0, y = 1, z = 2) in lexicographic order, with the corners p0 = the cube's corner,
 * p1 = p0 + e_a, p2 = p1 + e_b, p3 = p2 + e_c (neighbouring cubes split their common face alike, which makes the surface watertight).
 * A tetrahedron counts only if weight >= min_weight at its four corners.  Corner k is inside when tsdf < 0 (0 is outside); the four
 * bits select one of 16 cases with 0, 1 or 2 triangles (csrc/tsdf_tables.h, written by csrc/gen_tsdf_tables.py).  A volume with a
 * dimension of 1 has no cubes: nothing is written.
 *
 * fp_tsdf_emit_triangles: the triangles themselves.  offsets (int64, one per cube) is the exclusive prefix sum of counts and total
 * its sum; triangle offsets[c] + j is the j-th of cube c, in the order tetrahedron, then table order; so the output does not depend on
 * scheduling.  Per triangle corner (3 per triangle, rows 3 * t + k of the outputs), which lies on the grid edge between the voxels
 * a < b (linear indices):
 *   keys = a * 2^32 + b (int64);  t = fa / (fa - fb) with fa = tsdf[a], fb = tsdf[b];
 *   pos = pa + t * (pb - pa) per component (every tetrahedron sharing the edge computes the same bits);
 *   col = ca + t * (cb - ca) per channel when color_weight > 0 at both ends, the colour of the one end where it is, 128 otherwise;
 *   nrm = g / sqrtf((gx*gx + gy*gy) + gz*gz) with g = ga + t * (gb - ga) per component, or (0, 0, 1) unless that length is > 0.  The
 *     gradient of tsdf at a voxel is, per axis, 0.5f * (tsdf[i+1] - tsdf[i-1]) inside, tsdf[i+1] - tsdf[i] at the low face and
 *     tsdf[i] - tsdf[i-1] at the high face of the volume.
 * (v1 - v0) x (v2 - v0) points towards increasing tsdf (outwards).  A triangle whose index is not below total is not written.
 * No allocation, no host synchronisation; nothing is written outside the four outputs.
 * Argument errors (FP_ERR_INVALID_ARG): NULL origin; NULL depth / rgb / ob_in_cams / Ks with V > 0; a NULL volume array or output;
 * V outside 0..4096; H or W below 1 or more than 2^28 pixels; a dimension outside 1..FP_TSDF_MAX_DIM or more than 2^30 voxels; voxel or
 * trunc not finite or not > 0; min_depth or min_weight not finite; min_depth < 0; an origin that is not finite; total outside
 * 0..2^29. */
#define FP_TSDF_MAX_DIM 4096
int fp_tsdf_integrate(const float* depth /*dev V,H,W*/, const float* rgb /*dev V,H,W,3*/, const uint8_t* masks /*dev V,H,W|NULL*/,
                      const float* ob_in_cams /*dev V,16*/, const double* Ks /*dev V,9*/, int V, int H, int W, int nz, int ny, int nx,
                      const float* origin /*host 3*/, float voxel, float trunc, float min_depth, float* tsdf /*dev nz,ny,nx*/,
                      float* weight /*dev nz,ny,nx*/, float* color /*dev nz,ny,nx,3*/, float* color_weight /*dev nz,ny,nx*/, void* stream);
int fp_tsdf_count_triangles(const float* tsdf /*dev nz,ny,nx*/, const float* weight /*dev nz,ny,nx*/, int nz, int ny, int nx,
                            float min_weight, int32_t* counts /*dev (nz-1)(ny-1)(nx-1)*/, void* stream);
int fp_tsdf_emit_triangles(const float* tsdf /*dev*/, const float* weight /*dev*/, const float* color /*dev*/,
                           const float* color_weight /*dev*/, int nz, int ny, int nx, const float* origin /*host 3*/, float voxel,
                           float min_weight, const int64_t* offsets /*dev, one per cube*/, long long total, int64_t* keys /*dev 3*total*/,
                           float* pos /*dev 3*total,3*/, float* col /*dev 3*total,3*/, float* nrm /*dev 3*total,3*/, void* stream);
/* The surface components of a volume's cubes, for dropping floaters at extraction.  counts is fp_tsdf_count_triangles' output for a
 * volume of nz x ny x nx voxels: one int32 per cube, c = (cz * (ny-1) + cy) * (nx-1) + cx.
 *   A cube is active when counts[c] > 0.
 *   Two active cubes are adjacent when exactly one of cx, cy, cz differs, by 1: they share a face.
 *   A component is a maximal set of active cubes connected through adjacent pairs.
 *   labels[c] (int32) = the smallest cube index of c's component, or -1 for a cube that is not active.
 *   sizes[c] (int32) = the sum of counts over the component when labels[c] == c, and 0 everywhere else (an extraction has at most
 *     2^29 triangles, so it fits).
 * Faces are enough: two triangles that share a mesh edge lie in the same tetrahedron face, and that face belongs either to one cube or
 * to two face-adjacent cubes that both emitted triangles.  So every edge-connected piece of the mesh lies inside one component, and
 * dropping a component removes whole closed surfaces and opens nothing in what is kept.
 * Union-find over the cube array with integer atomics only (min and +), so both outputs have one value whatever the scheduling: the
 * definition's, bit for bit.  A volume with a dimension of 1 has no cubes: nothing is written.  No allocation, no host synchronisation
 * and no memset (every element of both outputs is written by the kernels; graph-capturable); nothing is written outside labels and
 * sizes.  The volume itself is not touched: fp_tsdf_raycast still sees what a dropped component was extracted from.
 * Argument errors (FP_ERR_INVALID_ARG), before any launch: a dimension outside 1..FP_TSDF_MAX_DIM or more than 2^30 voxels; NULL counts /
 * labels / sizes when there are cubes. */
int fp_tsdf_label_components(const int32_t* counts /*dev (nz-1)(ny-1)(nx-1)*/, int nz, int ny, int nx,
                             int32_t* labels /*dev, one per cube*/, int32_t* sizes /*dev, one per cube*/, void* stream);
/* The zero surface of a TSDF volume (the arrays, nz / ny / nx, origin and voxel of fp_tsdf_integrate) seen from N poses: per crop pixel
 * the depth, the camera-frame point, the camera-frame unit normal and the colour of the first crossing of tsdf from >= 0 to < 0 along the
 * pixel's ray.  The pixel convention is the rasteriser's (fp_render_crops), so depth / xyz / normal drop into fp_depth_agreement and
 * fp_icp_point_plane beside the same tf_to_crops as a render of the extracted mesh does.  Every operation is float32 without
 * contraction, one rounding per operation, in the order written; every 3-term sum is (a0*b0 + a1*b1) + a2*b2.
 * Per row n: T = poses[n] (object to camera, taken as rigid: R its 3x3 block, t its last column); {fx, skew, cx, fy, cy} from K (one
 * camera on the host, Ks NULL) or from Ks[view[n]] (the float32 table fp_render_crops takes, K NULL; view NULL means view 0, allowed
 * for V == 1); (umin, vmin, umax, vmax) = bbox2d[n], or (0, 0, W, H) with bbox2d NULL (which requires oh == H and ow == W).  The row is all
 * misses when one of T's 16 values, fx, fy, cx or cy is not finite, when the table's skew is not 0, when view[n] is outside 0..V-1, or
 * when the volume has a dimension of 1 (no cells).  Otherwise
 *   ax = (float)ow / (umax - umin),  ay = (float)oh / (vmax - vmin);   o_k = -((R0k*t0 + R1k*t1) + R2k*t2)   (o = -R^T t),
 * and per crop pixel (i, j), i along x:
 *   u = umin + ((float)i + 0.5f) / ax,  v = vmin + ((float)j + 0.5f) / ay   (full frame: exactly i + 0.5, j + 0.5);
 *   dc = ((u - cx) / fx, (v - cy) / fy, 1);   d_k = (R0k*dc.x + R1k*dc.y) + R2k   (d = R^T dc).
 * A point of the ray is o + z * d per component, z its camera depth.
 * Clipping: z0 = z_near, z1 = z_far; per axis a (x, y, z) with lo = origin_a and hi = origin_a + (float)(n_a - 1) * voxel:
 *   d_a == 0: the pixel is a miss unless lo <= o_a && o_a <= hi (inside that slab for every z);
 *   otherwise t1 = (lo - o_a) / d_a, t2 = (hi - o_a) / d_a, tmin = t1 < t2 ? t1 : t2, tmax = t1 < t2 ? t2 : t1,
 *     z0 = tmin > z0 ? tmin : z0,  z1 = tmax < z1 ? tmax : z1;
 * the pixel is a miss unless z0 <= z1.
 * March: samples k = 0, 1, ... at z_k = z0 + (float)k * step while z_k <= z1 (and k < FP_TSDF_RAYCAST_MAX_SAMPLES, which a rigid pose
 * never reaches: see the argument errors).  A sample: per axis q = ((o_a + z_k * d_a) - lo) / voxel, c_a = floorf(q), f_a = q - c_a.  It is
 * unknown unless 0 <= c_a <= n_a - 2 on every axis and weight >= min_weight at all eight corners of cell (c_x, c_y, c_z); otherwise its
 * value is the trilinear interpolation of tsdf: with lerp(a, b, t) = a + t * (b - a) and V[dx][dy][dz] the corner values,
 *   lerp(lerp(lerp(V000, V100, f_x), lerp(V010, V110, f_x), f_y), lerp(lerp(V001, V101, f_x), lerp(V011, V111, f_x), f_y), f_z).
 * An unknown sample forgets the previous one.  A known sample f < 0 ends the ray: as a hit when the sample before it was known (it
 * was >= 0: "0 is outside", as in the extraction), as a miss otherwise (the first known sample after the start or after an unknown
 * stretch: the surface is met from behind).  On a hit z* = z_prev + step * (f_prev / (f_prev - f)); there is no refinement sample.
 * Outputs on a hit: depth = z*; xyz = (z* * dc.x, z* * dc.y, z*); with q, c_a, f_a of the point o + z* * d as above, c_a clamped to
 * 0..n_a-2 (cf = floorf(q); cf = cf >= 0 ? cf : 0; cf = cf <= n_a-2 ? cf : n_a-2; f_a = q - cf) and the weights not consulted:
 *   normal: the gradient fp_tsdf_emit_triangles defines at each corner voxel, interpolated trilinearly per component as above, g;
 *     len = sqrtf((g.x*g.x + g.y*g.y) + g.z*g.z);  m = g / len per component;  normal_k = (Rk0*m.x + Rk1*m.y) + Rk2*m.z;  (0, 0, 0) unless
 *     len > 0 (the m.m > 0 test of fp_icp_point_plane then drops the pixel);
 *   color: over the corners in the order dx + 2 dy + 4 dz = 0..7 with color_weight > 0: w = (wx * wy) * wz with wx = dx ? f_x : 1 - f_x
 *     and likewise; acc = acc + w * color per channel, accw = accw + w (both from 0); color = acc / accw, or 128 unless accw > 0.
 * A miss writes 0 to every output.  Each of depth (N,oh,ow), xyz, normal, color (N,oh,ow,3) may be NULL; every element of the others is
 * written exactly once and nothing else is.  One lane per crop pixel, no atomics, no workspace, no allocation, no host synchronisation
 * (graph-capturable; origin and K are read during the call); every call repeats its bits, and a row has the bits of a call on it alone.
 * No index outside the volume is formed.  N == 0 does nothing.
 * Argument errors (FP_ERR_INVALID_ARG): a NULL volume array or origin; every output NULL; NULL poses with N > 0; a dimension outside
 * 1..FP_TSDF_MAX_DIM or more than 2^30 voxels; an origin that is not finite; voxel or step not finite or not > 0; z_near < 0,
 * z_far < z_near, or either not finite; min_weight not finite; N outside 0..65535; oh / ow / H / W below 1; more than 2^20 crop pixels;
 * bbox2d NULL with oh != H or ow != W; both or neither of K and Ks; a non-zero skew in K; view with K; V < 1 or view NULL with V > 1
 * (with Ks); a step so short that the volume's diagonal sqrt((nx-1)^2 + (ny-1)^2 + (nz-1)^2) * voxel holds more than
 * FP_TSDF_RAYCAST_MAX_SAMPLES - 2 of it (a ray's stretch inside the box is at most the diagonal, as |d| >= 1 for a rigid pose). */
#define FP_TSDF_RAYCAST_MAX_SAMPLES 65536
int fp_tsdf_raycast(const float* tsdf /*dev nz,ny,nx*/, const float* weight /*dev nz,ny,nx*/, const float* color /*dev nz,ny,nx,3*/,
                    const float* color_weight /*dev nz,ny,nx*/, int nz, int ny, int nx, const float* origin /*host 3*/, float voxel,
                    float min_weight, const float* poses /*dev N,16*/, const float* K /*host 9|NULL*/, const float* Ks /*dev V,9|NULL*/,
                    const int32_t* view /*dev N|NULL*/, int V, const float* bbox2d /*dev N,4|NULL*/, int H, int W, int N, int oh, int ow,
                    float step, float z_near, float z_far, float* depth /*dev N,oh,ow|NULL*/, float* xyz /*dev N,oh,ow,3|NULL*/,
                    float* normal /*dev N,oh,ow,3|NULL*/, float* color_out /*dev N,oh,ow,3|NULL*/, void* stream);
/* A texture atlas for a mesh from posed RGB-D reference views (those its TSDF volume was fused from): every texel is a point of one
 * face, coloured from the views that see it.  The atlas is per triangle: face f owns the T x T texel block at block column f % Bx and
 * block row f / Bx, so Wt = Bx * T, Ht = ceil(F / Bx) * T, and texel (i, j) of the block (i along x) is tex[(f / Bx) * T + j][(f % Bx) *
 * T + i].  The blocks with an index >= F (the rest of the last block row) get tex = 0 and coverage = 0; every texel of the atlas is
 * written and nothing else is.  A mesh samples the block through uv corners half a texel inside it: corner k of face f at
 * (((f % Bx) * T + 0.5 + dx_k) / Wt, ((f / Bx) * T + 0.5 + dy_k) / Ht) with (dx, dy) = (0, 0), (T-1, 0), (0, T-1), the row index growing
 * with v (the convention of fp_mesh_create), so that a bilinear tap inside the triangle reads the block's own texels only.
 * pos (Nv,3) and faces (F,3) are the mesh in the frame of the poses; vertex_color (Nv,3) in the units of rgb (NULL: 128) is what a
 * texel no view sees falls back to; the views are fp_tsdf_integrate's (depth, rgb, masks, ob_in_cams, Ks: prepared alike, K rounded to
 * float32; a view with a pose or intrinsic that is not finite, or with a skew, is skipped).  Every operation is float32 without
 * contraction, one rounding per operation, as parenthesised.  Per texel (f, i, j):
 *   a = (float)i / (float)(T-1), b = (float)j / (float)(T-1);  s = a + b;  if s > 1: a = a / s, b = b / s (a texel beyond the hypotenuse
 *     is a point on it: it holds the edge's colour for the taps that straddle the edge);  c = (1 - a) - b;
 *   p = (c*p0 + a*p1) + b*p2 per component, with p0, p1, p2 the face's vertices;
 *   n = (p1 - p0) x (p2 - p0): n.x = e1.y*e2.z - e1.z*e2.y, and cyclic;  nn = (n.x*n.x + n.y*n.y) + n.z*n.z;
 *   fallback = (c*col0 + a*col1) + b*col2 per channel, with 128 for the colour of a vertex whose index is outside 0..Nv-1; 128 without
 *     vertex_color.
 * A face with an index outside 0..Nv-1 or without nn > 0 && nn < infinity (no area, a vertex that is not finite) is unusable: its
 * texels get the fallback and coverage 0.  Otherwise the views are visited in index order; per view, with T its pose:
 *   X = ((T00*p.x + T01*p.y) + T02*p.z) + T03, Y and Z likewise from rows 1 and 2;  skip the view unless Z > 0;
 *   N = R n: N.x = (T00*n.x + T01*n.y) + T02*n.z, ...;  d = (N.x*X + N.y*Y) + N.z*Z;  NN = (N.x*N.x + N.y*N.y) + N.z*N.z;
 *   rr = (X*X + Y*Y) + Z*Z;  w = (d*d) / (NN*rr) (cos^2 of the angle between the normal and the ray);
 *   skip the view unless d < 0 (the face looks at the camera) and w >= min_cos*min_cos (not grazing);
 *   u = floorf(((fx * X) / Z + cx) + 0.5f), v likewise;  skip the view unless 0 <= u < W and 0 <= v < H (compared as floats);
 *   skip the view if mask[v][u] == 0;  dz = depth[v][u];  skip the view unless dz >= min_depth;
 *   skip the view unless fabsf(dz - Z) <= tol (another surface hides the texel in this view);
 *   per channel acc = acc + w * rgb[v][u];  accw = accw + w;  cnt = cnt + 1.
 * Then tex = cnt > 0 ? acc / accw : fallback and coverage = min(cnt, 255).  One texel per lane, the views inside the kernel in one
 * order: no atomics, no allocation, no host synchronisation (graph-capturable), every call repeats its bits.  No index outside pos,
 * faces, vertex_color or the frames is formed.  F == 0 does nothing.
 * Argument errors (FP_ERR_INVALID_ARG): NULL pos / faces / tex / coverage with F > 0; NULL depth / rgb / ob_in_cams / Ks with V > 0 (and
 * F > 0); T outside 2..FP_TEXTURE_BAKE_MAX_TEXELS; Bx < 1; Wt or Ht above FP_TEXTURE_BAKE_MAX_SIDE; F outside 0..2^24; Nv < 0; V outside
 * 0..4096; H or W below 1 or more than 2^28 pixels; tol or min_depth not finite or below 0; min_cos not in (0, 1]. */
#define FP_TEXTURE_BAKE_MAX_TEXELS 16
#define FP_TEXTURE_BAKE_MAX_SIDE 16384
int fp_texture_bake(const float* pos /*dev Nv,3*/, int Nv, const int32_t* faces /*dev F,3*/, int F,
                    const float* vertex_color /*dev Nv,3 in 0..255 | NULL*/, const float* depth /*dev V,H,W*/,
                    const float* rgb /*dev V,H,W,3 in 0..255*/, const uint8_t* masks /*dev V,H,W|NULL*/,
                    const float* ob_in_cams /*dev V,16*/, const double* Ks /*dev V,9*/, int V, int H, int W, int T, int Bx, float tol,
                    float min_cos, float min_depth, float* tex /*dev Ht,Wt,3*/, uint8_t* coverage /*dev Ht,Wt*/, void* stream);
/* ---- The crop stage: crop windows, render, warp and pose update of N hypotheses (estimater.py:250-268 track_one; several objects
 * and several camera frames per call).  The four entry points describe the scene with the same arguments:
 *   Camera, exactly one of
 *     K  (host 9): one camera for every hypothesis (f64 for fp_crop_windows, f32 for the others), with Ks = view = NULL and V = 0;
 *     Ks (dev V,9; same type as K), view (dev N int32, values 0..V-1, any order; NULL allowed only for V == 1: all 0) and V >= 1: a
 *        VIEW TABLE, hypothesis n has K = Ks[view[n]], with K = NULL.  Image inputs are then FRAME STACKS of V frames of one H x W,
 *        frame v at element offset (size_t)v * H * W * C, and hypothesis n reads frame view[n].
 *   Object, exactly one of
 *     mesh_diameter: one object, with diameters = obj = NULL and M = 0 (fp_render_crops: with `mesh`);
 *     diameters (dev M f64), obj (dev N int32, values 0..M-1, any order; NULL allowed only for M == 1: all 0) and M >= 1: hypothesis n
 *        has the diameter diameters[obj[n]] (fp_render_crops: and draws mesh obj[n] of `set`, whose size is M; mesh_diameter is
 *        not read).
 *   A view table goes with the diameter table (M == 1 and obj NULL for one object); Ks with a scalar mesh_diameter is refused.
 * Hypothesis n of a table call sees exactly what the one-camera, one-object call sees for frame view[n], K = Ks[view[n]], mesh
 * meshes[obj[n]] and the diameter diameters[obj[n]] (passed as that double to fp_crop_windows and rounded to float for the others):
 * the outputs are bit-identical.  An obj[n] outside 0..M-1 renders nothing and yields NaN-scaled values, never a memory access out of
 * the set.  A view[n] outside 0..V-1 never reads outside the stack or the table: the render draws nothing, the warp writes what a
 * pixel outside the frame gets, crop windows and pose update write NaN.
 * Argument errors (FP_ERR_INVALID_ARG, fp_last_error), checked in this order: N < 0; unknown flag bits (render, warp); a diameter
 * table that is NULL or has M < 1, obj NULL with M > 1; both K and a view table, a NULL K table or V < 1, view NULL with V > 1, a view
 * table without the diameter table; then N == 0 returns FP_OK; then neither K nor Ks (fp_pose_update: see there) and NULL tensors. */

/* Utils.py:577-621 compute_crop_window_tf_batch(method='box_3d') and the bbox of
 * predict_pose_refine.py:44-45 / predict_score.py:74-75 (closed-form inverse). */
int fp_crop_windows(const float* poses /*dev N,16*/, const double* K /*host 9|NULL*/, const double* Ks /*dev V,9|NULL*/,
                    const int32_t* view /*dev N|NULL*/, int V, double mesh_diameter, const double* diameters /*dev M|NULL*/,
                    const int32_t* obj /*dev N|NULL*/, int M, double crop_ratio, int out_w, int out_h, int N,
                    float* tf_to_crops /*dev N,9*/, float* bbox2d /*dev N,4*/, void* stream);

/* bytes of scratch fp_render_crops needs for (N hypotheses, V vertices, T triangles, oh x ow crops): per-hypothesis
 * vertex records (32 B/vertex) and per-strip triangle lists; caller-owned device memory, no alignment beyond 256 B */
size_t fp_workspace_bytes(int N, int V, int T, int oh, int ow);
/* bytes of LDS one workgroup of the rasteriser's third kernel (k_raster) asks for at launch, for crops `ow` pixels wide; host only.
 * Together with fp_conv3x3_sw_lds_bytes it must stay within the 160 KiB of a CU, so that a strip of the rasteriser of one
 * sub-batch stream fits beside a tile of the 3x3 convolution of another (tests/test_conv_sw_resources_host.py). */
size_t fp_raster_lds_bytes(int ow);

/* Utils.py:133-219 nvdiffrast_render (dr.rasterize + interpolate x5 + texture + Lambert shading + flips)
 * fused with predict_pose_refine.py:54-56 (*255), h5_dataset.py:79-114 (/255, xyz - t, 1/radius, masks)
 * and the channel concat of predict_pose_refine.py:187 (A = [rgb, xyz]).
 * Exactly one of `mesh` (with mesh_diameter; workspace: fp_workspace_bytes) and `set` (with obj and diameters, the meshes may
 * differ in V, T and texture / vertex colour; diameters may be NULL without FP_FLAG_NORMALIZE_XYZ; workspace:
 * fp_mesh_set_workspace_bytes(set, N, oh, ow)); a NULL set where obj, diameters or a view table ask for one is refused.
 * bbox2d NULL => full frame (needs oh=H, ow=W).  Any output may be NULL.
 *   A      (N,6,oh,ow) f32|f16 ; color (N,oh,ow,3) ; depth (N,oh,ow) ; xyz (N,oh,ow,3) ; normal (N,oh,ow,3)
 *   zbuf   (N,oh,ow) u32 fixed-point camera depth of the winner, FP_ZBUF_EMPTY if none ; tri_id i32, -1 if none */
int fp_render_crops(const fp_mesh* mesh /*|NULL*/, const fp_mesh_set* set /*|NULL*/, const int32_t* obj /*dev N|NULL*/,
                    const double* diameters /*dev M|NULL*/, float mesh_diameter, const float* poses /*dev N,16*/,
                    const float* bbox2d /*dev N,4|NULL*/, const float* K /*host 9|NULL*/, const float* Ks /*dev V,9|NULL*/,
                    const int32_t* view /*dev N|NULL*/, int V, int H, int W, int N, int oh, int ow, float w_ambient,
                    float w_diffuse, float xyz_thr, int flags, void* A /*dev*/, float* color /*dev*/, float* depth /*dev*/,
                    float* xyz /*dev*/, float* normal /*dev*/, uint32_t* zbuf /*dev*/, int32_t* tri_id /*dev*/,
                    void* workspace /*dev*/, size_t workspace_bytes, void* stream);

/* kornia warp_perspective call sites predict_pose_refine.py:63,72 / predict_score.py:89,90 fused with
 * h5_dataset.py:79-114 (refine) or :137-170 (score: depth crop -> frame -> back-projection -> crop) and
 * the concat of predict_pose_refine.py:188 (B = [rgb, xyz]).
 * rgb (H,W,3) f32 in 0..255; xyz_map (H,W,3) f32 (REFINE); depth (H,W) f32 (SCORE); with a view table each is a (V,...) stack. */
int fp_warp_crops(const float* rgb /*dev*/, const float* xyz_map /*dev|NULL*/, const float* depth /*dev|NULL*/,
                  const float* tf_to_crops /*dev N,9*/, const float* K /*host 9|NULL*/, const float* Ks /*dev V,9|NULL*/,
                  const int32_t* view /*dev N|NULL*/, int V, const float* poses /*dev N,16*/, float mesh_diameter,
                  const double* diameters /*dev M|NULL*/, const int32_t* obj /*dev N|NULL*/, int M, int flags, int mode, int H,
                  int W, int N, int oh, int ow, void* B /*dev N,6,oh,ow*/, void* stream);

/* predict_pose_refine.py:195-234 + Utils.py:848-855 + pytorch3d so3_exp_map / rotation_6d_to_matrix.
 * trans_delta_out / rot_delta_out (optional): the metric translation delta and the applied rotation matrix
 * (so3_exp_map(.)^T), i.e. what the reference keeps in last_trans_update / last_rot_update (:238-239).
 * poses_in and poses_out MUST NOT OVERLAP: the kernel holds both as __restrict__, there is no in-place update.  Exactly rows
 * 0..N-1 of each given output are written; N == 0 writes nothing.
 * The camera is read by trans_rep deepim only (with tf_to_crops and input_w, the crop width): without a view table K may be NULL
 * for the other trans_reps; a view table, once any of Ks / view / V is given, is required whole whatever trans_rep.
 * An obj[n] outside 0..M-1 reads no diameter: it counts as NaN, so with normalize_xyz the translation column of poses_out row n and
 * trans_delta_out row n are NaN (the rotation block is what it is for any diameter); without normalize_xyz the diameter is not
 * used and the row is the scalar form's.  A view[n] outside 0..V-1: all of poses_out row n (16 values) and of the given
 * trans_delta_out / rot_delta_out rows n are NaN, whatever trans_rep. */
int fp_pose_update(const float* trans /*dev N,3*/, const float* rot /*dev N,3|6*/, const float* poses_in /*dev N,16*/,
                   int rot_rep, int normalize_xyz, const float* trans_normalizer /*host 3*/, float rot_normalizer,
                   float mesh_diameter, const double* diameters /*dev M|NULL*/, const int32_t* obj /*dev N|NULL*/, int M, int N,
                   float* poses_out /*dev N,16*/, float* trans_delta_out /*dev N,3|NULL*/, float* rot_delta_out /*dev N,9|NULL*/,
                   int trans_rep, const float* K /*host 9|NULL*/, const float* Ks /*dev V,9|NULL*/,
                   const int32_t* view /*dev N|NULL*/, int V, const float* tf_to_crops /*dev N,9|NULL (deepim)*/,
                   float input_w /*crop width (deepim)*/, void* stream);

/* ---- network stage.  Arithmetic policy of every entry point below = the op sequence torch.cuda.amp.autocast(fp16)
 * produces for the reference's modules (predict_pose_refine.py:190-191, predict_score.py:193-194): fp16 operands,
 * fp32 accumulation, and a rounding to fp16 wherever the reference holds an fp16 tensor. ---- */

/* refine_network.py:38 / score_network.py:37 first ConvBNReLU (7x7, stride 2, pad 3, 6 -> 64): the "patch-embed conv"
 * as an MFMA implicit GEMM.  x (B,6,Hin,Win) f16 NCHW; w (64, 6*7*7) f16 row-major (PyTorch conv weight flattened);
 * bias (64) f32 holding fp16-representable values | NULL; bn_scale/bn_shift (64) f32 | NULL: eval BatchNorm2d as
 * x*scale + shift.  y = relu(f16(f16(f16(conv) + bias) * scale + shift)), NHWC inside a (B, Hin/2 + 2 pad, Win/2 + 2 pad, 64)
 * f16 buffer whose `pad`-pixel border (pad = 0 | 1) the kernel does not touch (pad 1 = the input layout of fp_igemm_f16_fwd). */
int fp_conv7x7s2_bn_relu_fwd(const void* x /*dev*/, const void* w /*dev*/, const float* bias /*dev|NULL*/,
                             const float* bn_scale /*dev|NULL*/, const float* bn_shift /*dev|NULL*/, void* y /*dev*/,
                             int B, int Hin, int Win, int pad, void* stream);

/* Addressing of one operand of fp_igemm_f16_fwd: GEMM row m = (image b, oy, ox) with b = m / pixels_per_image,
 * oy = (m % pixels_per_image) / width, ox = ... % width, lives at element offset
 *   (((b' * padded_h + oy*stride + offset) * padded_w + ox*stride + offset) * cstride + coff + cg * cgroup
 * of an NHWC fp16 buffer with a zero border, where (b', cg) = (b % bsplit, b / bsplit) if bsplit > 0 else (b, 0)
 * (bsplit writes the A- and B-image features of a pair side by side along C: the channel concat of
 * refine_network.py:82-85 / score_network.py:66-69 without a copy).  A plain matrix is {1,1,1,1,1,0,ld,0,0,0}. */
typedef struct {
  int pixels_per_image, width, padded_h, padded_w, stride, offset, cstride, coff, bsplit, cgroup;
} fp_igemm_geom;

#define FP_IGEMM_RELU 1      /* ReLU after the residual add */
#define FP_IGEMM_HAS_W_TILES 4 /* the struct has the trailing member w_tiles and the library may read it (ABI 213: a caller compiled
                                 against the ABI-211 header passes a shorter struct, never sets the bit, and is never read past its end) */
#define FP_IGEMM_ROUND_ACC 2 /* nn.Conv2d semantics: the accumulator is rounded to fp16 BEFORE the bias is added (ATen adds the
                                bias to the fp16 convolution output) and BatchNorm, if given, rounds once more; without the
                                flag: nn.Linear semantics, one rounding of accumulator + bias */

/* Which MFMA instruction the main loop of the shifted-window 3x3 kernel (csrc/conv_sw.hip, ping-pong schedule) runs on: 32 v_mfma_f32_16x16x32_f16
 * or 16 v_mfma_f32_32x32x16_f16 per wave and k-step.  The same products with the same rounding points; the order of the fp32 sums inside an
 * MFMA is the hardware's, so the two are specified to agree up to summation order (on gfx950 they were measured to agree bit for bit).  Neither bit: the library's default (16x16x32); both: refused.
 * Ignored by the launches that do not reach that kernel. */
#define FP_IGEMM_MFMA_16X16X32 16
#define FP_IGEMM_MFMA_32X32X16 32

/* fp_igemm_f16_fwd compiles the epilogue of the layer kinds the networks launch (conv rounding + bias + ReLU, with or without BatchNorm,
 * residual, positional second output) as bodies of their own, chosen per launch from the members below; every other combination runs one
 * generic body that reads them at run time.  With this bit a launch runs the generic body whatever its kind: the same arithmetic in the
 * same order, hence the same bits -- the A/B arm of that specialisation (tests/test_gpu_igemm_epilogue_modes.py) and nothing a product
 * call needs.  Ignored by fp_igemm_f16_splitk_fwd, whose epilogue is a kernel of its own. */
#define FP_IGEMM_EPILOGUE_GENERIC 64

/* The shifted-window 3x3 kernel's 512 x 128 tile stored straight from the accumulators (csrc/conv_sw.hip k_conv_sw_direct): the 16x16x32
 * MFMAs are issued with pixels as A and weights as B, a lane then owns four consecutive channels of a pixel and stores them as they are
 * converted, without the transposition through LDS.  The same products in the same k order and the same epilogue statements per element
 * (measured on gfx950: the same bits).  Taken by the launches that kernel exists for -- that tile, 16x16x32 MFMAs, conv rounding + bias +
 * ReLU with or without BatchNorm and residual, no positional output, not FP_IGEMM_EPILOGUE_GENERIC -- and ignored by every other one.
 * FP_IGEMM_W_TILES_DIRECT: w_tiles comes from fp_pack_conv3x3_tiles_direct_f16, the row order of that kernel.  A launch that reads w_tiles
 * refuses the layout of the other kernel (FP_ERR_INVALID_ARG). */
/* (flag values 8 and 128 are not assigned: the library refuses them as unknown, which tests/test_abi.py and
 * tests/test_gpu_igemm_epilogue_modes.py rely on) */
#define FP_IGEMM_DIRECT_STORE 256
#define FP_IGEMM_W_TILES_DIRECT 512

/* What fp_igemm_f16_fwd does with the fp32 accumulators (all members optional; NULL struct = plain fp16 store) */
typedef struct {
  const float* bias;           /* dev (N) f32 | NULL; for conv semantics fp16-representable values */
  const float* bn_scale;       /* dev (N) f32 | NULL: eval BatchNorm2d as x*scale + shift (needs FP_IGEMM_ROUND_ACC) */
  const float* bn_shift;
  const void* residual;        /* dev fp16 | NULL: `out += identity` (network_modules.py:107), rounded to fp16 */
  const fp_igemm_geom* r_geom; /* host: addressing of the residual */
  int flags;                   /* FP_IGEMM_RELU | FP_IGEMM_ROUND_ACC | FP_IGEMM_HAS_W_TILES | FP_IGEMM_MFMA_* | FP_IGEMM_EPILOGUE_GENERIC | FP_IGEMM_DIRECT_STORE | FP_IGEMM_W_TILES_DIRECT */
  const float* pe;             /* dev (pe_period, N) f32 | NULL: second output y_pe[m, n] = f16(f32(y[m, n]) + pe[m % pe_period, n]), */
  int pe_period;               /*   the PositionalEmbedding add of network_modules.py:133-137 fused into the last conv of the */
  void* y_pe;                  /*   encoder; y_pe is a plain (M, N) fp16 matrix */
  const void* w_tiles;         /* dev | NULL (since ABI 212; read only with FP_IGEMM_HAS_W_TILES): the SAME weights once more, in the tile-packed layout of fp_pack_conv3x3_tiles_f16; */
                               /*   the shifted-window 3x3 kernel then fetches a k-step's 128 x 32 weight tile as one contiguous 8 KiB run */
} fp_igemm_epilogue;

/* network_modules.py:37-50 ConvBNReLU / :73-111 ResnetBasicBlock (3x3, pad 1, stride 1|2, eval BatchNorm) and the
 * 512-wide Linear layers of refine_network.py:56-70 / score_network.py:52-53, as ONE MFMA implicit GEMM:
 *   acc[m, n] = sum_{tap, ci} x[row(m) + tap][ci] * w[n][tap*Cin + ci]                       (fp32 accumulation)
 *   y = act( f16(epilogue(acc)) (+ residual[m, n], rounded to f16) ),  epilogue per fp_igemm_epilogue.
 * x / y / residual: NHWC fp16 addressed by their fp_igemm_geom (the input's border must be zero; its geometry
 * addresses tap (0,0), i.e. offset = 0 for pad 1); w (N, taps*Cin) fp16 with k ordered (ky, kx, ci).
 * taps = 9 (3x3) or 1 (GEMM); N % 128 == 0; Cin % 64 == 0.  Stride-1 3x3 convolutions over one padded grid run the
 * shifted-window kernel (csrc/conv_sw.hip), everything else the generic implicit GEMM. */
int fp_igemm_f16_fwd(const void* x /*dev*/, const fp_igemm_geom* x_geom /*host*/, const void* w /*dev*/, void* y /*dev*/,
                     const fp_igemm_geom* y_geom /*host*/, int M, int N, int Cin, int taps,
                     const fp_igemm_epilogue* epilogue /*host|NULL*/, void* stream);

/* One-time repack of a 3x3 convolution weight (N, 9*Cin) fp16, k ordered (ky, kx, ci), for fp_igemm_epilogue.w_tiles: per block of 128
 * output channels and per k-step s = (32-channel chunk cc, tap) in the order the shifted-window kernel consumes them (s = 9 cc + tap), the
 * 128 x 32 weight tile as the 8 KiB LDS image of that kernel (rows of 64 B, 16-byte chunk c of row r at position c ^ ((r >> 2) & 3)):
 *   w_tiles[((bn * 9 * Cin / 32 + s) * 128 + r) * 32 + 8 * pc + e] = w[128 bn + r][tap * Cin + 32 cc + 8 * (pc ^ ((r >> 2) & 3)) + e].
 * N % 128 == 0, Cin % 32 == 0; w_tiles has the size of w and must not alias it.  No reference counterpart (a layout, not an operation). */
int fp_pack_conv3x3_tiles_f16(const void* w /*dev*/, void* w_tiles /*dev*/, int N, int Cin, void* stream);
/* The same repack for FP_IGEMM_DIRECT_STORE launches (flag FP_IGEMM_W_TILES_DIRECT): row r of a 128-channel tile holds weight row
 *   rho(r) = (r & 64) + 4 * (4 * tau((r >> 2) & 3) + (r & 3)) + ((r >> 4) & 3),  tau = (0, 3, 1, 2),
 * of that tile, its chunks where the layout above puts them (by r, not by rho(r)):
 *   w_tiles[((bn * 9 * Cin / 32 + s) * 128 + r) * 32 + 8 * pc + e] = w[128 bn + rho(r)][tap * Cin + 32 cc + 8 * (pc ^ ((r >> 2) & 3)) + e]. */
int fp_pack_conv3x3_tiles_direct_f16(const void* w /*dev*/, void* w_tiles /*dev*/, int N, int Cin, void* stream);
/* bytes of LDS one workgroup of the shifted-window 3x3 convolution (512 x 128 tiles, every product layer) asks for at launch; host only */
int fp_conv3x3_sw_lds_bytes(void);

/* fp_igemm_f16_fwd for launches of a few dozen tiles -- the reference's tracking call (estimater.py:250-268: ONE hypothesis, so the
 * 512 -> 512 convolutions are 400 x 512 x 4608 products = 16 tiles on 256 CUs, each running its whole k loop): the k range is cut into
 * `splits` contiguous pieces of whole 64-wide k-steps, workgroup (tile, piece) leaves fp32 partial accumulators in `workspace`, and a
 * second launch adds the pieces IN ORDER and applies the epilogue (same operations per element as fp_igemm_f16_fwd).  Deterministic;
 * another fp32 summation order than fp_igemm_f16_fwd's, so equal to it up to summation order, not bit for bit -- a caller that
 * needs the bits of a larger batch (shards, sub-batches) must not mix the two for one layer.  Arguments as fp_igemm_f16_fwd;
 * 1 <= splits <= taps * Cin / 64; workspace: fp_igemm_splitk_workspace_bytes(M, N, splits) bytes of device scratch, 16-byte aligned. */
size_t fp_igemm_splitk_workspace_bytes(int M, int N, int splits);
int fp_igemm_f16_splitk_fwd(const void* x /*dev*/, const fp_igemm_geom* x_geom /*host*/, const void* w /*dev*/, void* y /*dev*/,
                            const fp_igemm_geom* y_geom /*host*/, int M, int N, int Cin, int taps,
                            const fp_igemm_epilogue* epilogue /*host|NULL*/, int splits, void* workspace /*dev*/,
                            size_t workspace_bytes, void* stream);

/* network_modules.py:133-137 PositionalEmbedding as the in_proj operand: out = f16(f32(tok) + pe[row % S]).
 * tok / out (M, D) fp16, pe (S, D) f32; D must be 512.  (The fp32 sum itself is never stored: fp_layernorm_res_fwd
 * recomputes it.) */
int fp_add_pe_f16_fwd(const void* tok /*dev*/, const float* pe /*dev*/, void* out /*dev*/, int M, int S, int D, void* stream);

/* refine_network.py:82-85 `ab = torch.cat((a, b), 1)` when every b is ONE image -- the first refine iteration of
 * estimater.py:214-215 register(), whose hypotheses share a translation (estimater.py:132-133) and therefore the observed
 * crop: dst[c][r][0..channels) = src[r][0..channels) for c < copies.  fp16 rows at row strides (in fp16 values; channels and
 * all strides multiples of 8, pointers 16-byte aligned), copy c at dst + c * dst_copy_stride.  src and dst may be
 * different images of one buffer as long as the source rows are not among the destination rows. */
int fp_replicate_rows_f16(const void* src /*dev*/, void* dst /*dev*/, int copies, int rows, int channels, int src_row_stride,
                          int dst_row_stride, long long dst_copy_stride, void* stream);

/* fp_replicate_rows_f16 per segment, in place: several (camera, object) groups in the first refine iteration of a batched
 * registration, each with its own shared observed crop.  buf points at channel c0 of pixel 0 of image 0; image i, pixel p is at
 * buf + i * image_stride + p * pixel_stride (fp16 values).  Segment s (images seg_offsets[s] .. seg_offsets[s+1]-1, dev int32
 * S+1) gets `channels` values of image s at every pixel: the sources are images 0..S-1, which are destinations too, and each is
 * read before it is overwritten.  Every segment must hold at least one image (offsets from 0, strictly increasing); offsets are
 * clamped to 0..images.  channels and strides multiples of 8, buf 16-byte aligned, segments <= images. */
int fp_replicate_segments_f16(void* buf /*dev*/, const int32_t* seg_offsets /*dev S+1*/, int segments, int images, int pixels,
                              int channels, int pixel_stride, long long image_stride, void* stream);

/* The LayerNorms of nn.TransformerEncoderLayer (refine_network.py:56-70; post-norm, eps 1e-5) on the fp32 residual
 * stream autocast keeps:  z = resid + f32(branch16);  y = LN(z)*gamma + beta  -> y32 (M,D) f32 and/or y16 (M,D) f16,
 * with resid = x32 (M,D) f32, or f32(tok16) + pe[row % S] when x32 is NULL.  D must be 512. */
int fp_layernorm_res_fwd(const float* x32 /*dev|NULL*/, const void* tok16 /*dev|NULL*/, const float* pe /*dev|NULL*/, int S,
                         const void* branch16 /*dev*/, const float* gamma /*dev D*/, const float* beta /*dev D*/, float eps,
                         float* y32 /*dev|NULL*/, void* y16 /*dev|NULL*/, int M, int D, void* stream);

/* Fragment-packed copy of a (512, 512) fp16 weight matrix W[out][in] (nn.Linear layout) for fp_linear_layernorm_fwd and
 * fp_ffn_layernorm_mean_fwd, whose waves read their weight rows straight from L2 into MFMA operand registers: for channel group
 * w = out / 64, k16-step q = in / 16, channel tile i = (out / 32) % 2 the 64 lanes' operands stand back to back,
 *   packed[((w * 32 + q) * 2 + i) * 64 + lane][0..7] = W[64 w + 32 i + (lane & 31)][16 q + 8 (lane >> 5) + 0..7],
 * so a wave load is one contiguous KiB (the row-per-lane form of the same load is served at one lane per clock by the vector
 * cache).  Same size as the matrix; done once per weight matrix; `packed` must not alias `w16`. */
int fp_pack_linear512_f16(const void* w16 /*dev*/, void* packed /*dev*/, void* stream);

/* y16 (M, N) = f16(x16 (M, 512) @ W^T + bias) [ReLU if relu != 0]: nn.Linear under autocast (fp16 operands, fp32 accumulation +
 * bias, one rounding) for in_features = 512 and N = 512 n <= 3072 output features -- the in_proj of nn.MultiheadAttention (N = 1536;
 * refine_network.py:56-70 through nn.TransformerEncoderLayer, score_network.py:52-53,73,86).  The bits of fp_igemm_f16_fwd with
 * taps = 1 (same k order per accumulator); a workgroup fetches its 128 x 512 input tile once and keeps it in LDS for all N / 512
 * column blocks, weights from L2 into registers.  w_packed: the N / 512 blocks of 512 output channels of W (N, 512), each through
 * fp_pack_linear512_f16, back to back; bias (N) f32 | NULL. */
int fp_linear512_f16_fwd(const void* x16 /*dev*/, const void* w_packed /*dev*/, const float* bias /*dev|NULL*/, void* y16 /*dev*/,
                         int M, int N, int relu, void* stream);

/* fp_pack_linear512_f16 in the row order of the direct-store kernel of fp_linear512_flags_f16_fwd: within every group of 64 output
 * channels, packed row 32 i + c holds weight row 2 c + i (i = 0 | 1, c < 32), i.e.
 *   packed[((w * 32 + q) * 2 + i) * 64 + lane][0..7] = W[64 w + 2 (lane & 31) + i][16 q + 8 (lane >> 5) + 0..7]. */
int fp_pack_linear512_direct_f16(const void* w16 /*dev*/, void* packed /*dev*/, void* stream);

/* fp_linear512_f16_fwd with flags instead of `relu`.  FP_LINEAR512_DIRECT_STORE: the kernel that exchanges the two MFMA sources, so that
 * a lane owns two adjacent output channels and every tile leaves from the accumulators as whole 128-byte lines, without a transposition
 * through LDS; the same dot products in the same k order and the same rounding, i.e. the same bits; needs M * N * 2 < 2^31.
 * FP_LINEAR512_W_DIRECT: w_packed comes from fp_pack_linear512_direct_f16.  The two go together: a launch whose kernel cannot read the
 * order of its pack is refused. */
#define FP_LINEAR512_RELU 1
#define FP_LINEAR512_DIRECT_STORE 2
#define FP_LINEAR512_W_DIRECT 4
int fp_linear512_flags_f16_fwd(const void* x16 /*dev*/, const void* w_packed /*dev*/, const float* bias /*dev|NULL*/, void* y16 /*dev*/,
                               int M, int N, int flags, void* stream);

/* A 512 -> 512 nn.Linear of the encoder layer (refine_network.py:56-70: self_attn.out_proj or linear2, under autocast: fp16
 * operands, fp32 accumulation + bias, one rounding to fp16) fused with the residual add and the LayerNorm that consume it:
 * fp_igemm_f16_fwd (taps = 1, N = 512) followed by fp_layernorm_res_fwd with branch16 = that product, in one launch and
 * without the (M, 512) product reaching HBM; per element the same instruction sequence, i.e. the same bits.
 * x16 (M, 512) fp16, w16_packed = fp_pack_linear512_f16 of the (512, 512) weight, bias (512) f32 | NULL; K and D must be 512 (the
 * 128 x K A tile of a workgroup lives in LDS whole); the other arguments as fp_layernorm_res_fwd.  ldx (ABI 213): x16 may be a column
 * block of a wider matrix -- one head's (M, 512) half of the (M, 1024) output of a two-head fp_attention_f16_fwd call (round 6: the
 * self-attention of RefineNet's trans_head and rot_head, refine_network.py:56-70, as one 8-head launch). */
int fp_linear_layernorm_fwd(const void* x16 /*dev*/, const void* w16_packed /*dev*/, const float* bias /*dev|NULL*/,
                            const float* x32 /*dev|NULL*/, const void* tok16 /*dev|NULL*/, const float* pe /*dev|NULL*/, int S,
                            const float* gamma /*dev D*/, const float* beta /*dev D*/, float eps, float* y32 /*dev|NULL*/,
                            void* y16 /*dev|NULL*/, int M, int K, int D, int ldx /* row stride of x16 in fp16 values; 0 = K */,
                            void* stream);

/* Everything of nn.TransformerEncoderLayer behind the attention context (refine_network.py:56-70: self_attn.out_proj, `x + sa`, norm1,
 * linear1 -> ReLU -> linear2, `x + ff`, norm2) + the token mean of RefineNet.forward (refine_network.py:90-91), in ONE launch (+ the
 * finish kernel) = fp_linear_layernorm_fwd followed by fp_ffn_layernorm_mean_fwd, with norm1's fp16 output staying in LDS between them
 * (round 6; the same bits as those two calls: per element the same instruction sequences).  ctx16: (M, 512) fp16 with row stride ldx
 * (0 = 512), M = groups * rows_per_group; tok16 (M, 512) fp16 + pe (rows_per_group, 512) f32 = the layer input f32(tok16) + pe[row %
 * rows_per_group]; *_packed: fp_pack_linear512_f16 of the three (512, 512) weights; out (groups, 512) f32.  workspace:
 * fp_encoder_tail_workspace_bytes(groups, rows_per_group) bytes of device scratch (norm1's fp32 output -- the residual of norm2 -- and
 * the token-mean chunk sums), 16-byte aligned. */
size_t fp_encoder_tail_workspace_bytes(int groups, int rows_per_group);
int fp_encoder_tail_mean_fwd(const void* ctx16 /*dev*/, int ldx, const void* wo_packed /*dev*/, const float* bo /*dev|NULL*/,
                             const void* tok16 /*dev*/, const float* pe /*dev*/, const float* gamma1 /*dev*/, const float* beta1 /*dev*/,
                             const void* w1_packed /*dev*/, const float* b1 /*dev|NULL*/, const void* w2_packed /*dev*/,
                             const float* b2 /*dev|NULL*/, const float* gamma2 /*dev*/, const float* beta2 /*dev*/, float eps,
                             float* out /*dev*/, void* workspace /*dev*/, size_t workspace_bytes, int groups, int rows_per_group,
                             void* stream);

/* The feed-forward half of nn.TransformerEncoderLayer (refine_network.py:56-70: linear1 -> ReLU -> linear2, `x + ff`, norm2; under
 * autocast: fp16 Linears with fp32 accumulation + bias and one rounding each, fp32 residual stream and LayerNorm) fused with the
 * token mean that follows it in RefineNet.forward (refine_network.py:90-91, taken before the 512 -> 3|6 head: the mean and that
 * Linear commute):  out[g, :] = mean_{r < rows_per_group} ( LN(x32[row] + f32(linear2(relu(linear1(y16[row]))))) * gamma + beta ),
 * row = g * rows_per_group + r.  = fp_igemm_f16_fwd x 2 + fp_colmean_f16_fwd with neither (M, 512) intermediate reaching HBM:
 * a workgroup owns 128 complete rows through both Linears and the LayerNorm; the token mean is summed in chunks of 16
 * consecutive rows of a group, then over a group's chunks in order -- deterministic, and independent of where in the batch a
 * group sits (a sub-batch or shard returns the bits of the full batch); another fp32 summation order than fp_colmean_f16_fwd's, so
 * equal to it up to fp32 rounding, not bit for bit.  y16 (M, 512) fp16 = norm1's output, x32 (M, 512) f32 = the residual stream,
 * w1_packed / w2_packed = fp_pack_linear512_f16 of the (512, 512) fp16 weights, b1 / b2 (512) f32 | NULL, out (groups, 512) f32,
 * M = groups * rows_per_group, rows_per_group a multiple of 16.
 * workspace: M / 16 * 512 floats of device scratch owned by the caller. */
int fp_ffn_layernorm_mean_fwd(const void* y16 /*dev*/, const void* w1_packed /*dev*/, const float* b1 /*dev|NULL*/,
                              const void* w2_packed /*dev*/, const float* b2 /*dev|NULL*/, const float* x32 /*dev*/,
                              const float* gamma /*dev 512*/, const float* beta /*dev 512*/, float eps, float* out /*dev*/,
                              float* workspace /*dev*/, size_t workspace_bytes, int groups, int rows_per_group, void* stream);

/* `.mean(dim=1)` over the tokens of each hypothesis (refine_network.py:90-91, score_network.py:74), optionally fused
 * with the residual add + LayerNorm that precede it: out[g, :] = mean_{r < rows_per_group} f(row g*rows_per_group + r),
 * f = LN(resid32 + f32(x))*gamma + beta if gamma != NULL (resid32 may be NULL) else f32(x).  x (groups*rows_per_group, D)
 * fp16, resid32 same shape f32, out (groups, D) f32. */
int fp_colmean_f16_fwd(const void* x /*dev*/, const float* resid32 /*dev|NULL*/, const float* gamma /*dev D|NULL*/,
                       const float* beta /*dev D|NULL*/, float eps, float* out /*dev*/, int groups, int rows_per_group,
                       int D, void* stream);

#define FP_ROWS_ROUND_F16 1 /* y (f32) holds fp16-representable values: the reference keeps these outputs in fp16 */
#define FP_ROWS_X_F16 2     /* x is fp16 instead of f32 */
#define FP_ROWS_Y_F16 4     /* y is stored as fp16 instead of f32 */

/* The Linear layers that follow a token mean (refine_network.py:58,69 heads; score_network.py:53 out_proj after the
 * mean has been commuted in front of it; score_network.py:57 final Linear): y[M,N] = x[M,K] @ w[N,K]^T + bias for a
 * few hundred rows, fp32 accumulation.  x f32|f16, w f16, bias f32|NULL, y f32|f16.  K % 8 == 0, K <= 2048. */
int fp_rows_linear_fwd(const void* x /*dev*/, const void* w /*dev*/, const float* bias /*dev|NULL*/, void* y /*dev*/,
                       int M, int K, int N, int flags, void* stream);

#define FP_ATT_FP16_SCORES 1 /* the need_weights=True branch of F.multi_head_attention_forward under autocast
                                (score_network.py:73,86): q * sqrt(1/d) rounded to fp16 and the q.k scores rounded to fp16
                                before the fp32 softmax; default: F.scaled_dot_product_attention (fp32 scores) */

/* The attention core of nn.MultiheadAttention(512, 4) as the networks call it (query = key = value, no mask, eval):
 * refine_network.py:56-70 (nn.TransformerEncoderLayer self-attention over the 400 tokens of a hypothesis),
 * score_network.py:52-53 (token attention) and :84-88 (attention across the hypotheses), i.e. what
 * torch.nn.functional.multi_head_attention_forward does between in_proj and out_proj:
 *   out[b, t, h*hd:(h+1)*hd] = softmax_t'(q[b,t,h,:] . k[b,t',h,:] / sqrt(hd)) v[b,t',h,:]
 * qkv (B*S, 3*H*hd) fp16 = the in_proj output [q | k | v]; out (B*S, H*hd) fp16 = the out_proj input.  hd must be 128, and
 * the rows of one sequence must lie within 2 GiB of qkv: max(S, 64) * 3*H*hd * 2 bytes <= 2^31 - 1 (refused otherwise).
 * fp32 softmax statistics and accumulation, probabilities rounded to fp16 for the second product, normalisation
 * after it (flash-attention order); the (B*H, S, S) probability tensor is never formed. */
int fp_attention_f16_fwd(const void* qkv /*dev*/, void* out /*dev*/, int B, int S, int H, int head_dim, int flags,
                         void* stream);

/* fp_attention_f16_fwd over B sequences of DIFFERENT lengths packed row after row (the scorer's cross-hypothesis attention of
 * several objects in one call, score_network.py:83-88 per object): sequence b is rows seg_offsets[b] .. seg_offsets[b+1] - 1 of qkv
 * (Ntot, 3*H*hd) and of out (Ntot, H*hd); no attention crosses a segment boundary.  seg_offsets (B+1) int32 stays on the device
 * (non-decreasing, seg_offsets[0] = 0 -- the caller's to guarantee); max_S is a host bound on every segment's length that
 * sizes the grid and is held to the 2 GiB span limit of S above.  Segments of length 0 write nothing.  Arithmetic and flags as
 * fp_attention_f16_fwd: every segment gets the bits of fp_attention_f16_fwd(B=1, S=its length) on its rows. */
int fp_attention_segments_f16_fwd(const void* qkv /*dev Ntot,3*H*hd*/, void* out /*dev Ntot,H*hd*/,
                                  const int32_t* seg_offsets /*dev B+1*/, int B, int max_S, int H, int head_dim, int flags,
                                  void* stream);

/* mycpp/src/app/pybind_api.cpp:24-68 cluster_poses (host, init-time). Returns #kept, indices in keep_idx. */
int fp_cluster_poses(float angle_diff_deg, float dist_diff, const float* poses /*host N,16*/, int N,
                     const float* symmetry_tfs /*host S,16*/, int S, int* keep_idx /*host N*/);

#ifdef __cplusplus
}
#endif
#endif /* FP_AMD_H */
