/*
 * tactile_gym_hip_test.h - C ABI of libtactile_gym_hip_test.so: device self-tests of pieces of the product's kernels.
 *
 * TEST INFRASTRUCTURE, not part of the boundary a maintainer binds (that is tactile_gym_hip.h / libtactile_gym_hip.so): built by
 * csrc/build.sh next to the product library from the same device headers, loaded only by tests/ (tactile_gym_amd._capi.test_lib()).
 * Translation units: tg_narrow_test.hip, tg_selftest.hip, tg_physics_test.hip, tg_state_test.hip, tg_render_test.hip, tg_scene_test.hip and
 * tg_stack_test.hip, the last three linked with the product's own tg_raster.o, tg_scene.o and tg_stack.o.
 * Every function returns 0 on success, -1 bad argument, -2 no HIP device / allocation failed, -3 launch failed (tg_selftest_stack: the
 * launcher's own value).
 */
#ifndef TACTILE_GYM_HIP_TEST_H
#define TACTILE_GYM_HIP_TEST_H

#include <stdint.h>

#include "tactile_gym_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Self-test of the wave-mapped GJK / EPA (tg_config.narrowphase; csrc/tg_narrowphase.hpp) on n_cases placements of a convex hull against the
 * box of half extents half[3]: hulls [n_cases][n_hull][3] in the box frame (n_hull <= 1152); out [n_cases][11] = found (1 / 0), signed core
 * distance (< 0: overlap depth), unit normal from the box to the hull, witness point on the hull, witness point on the box. */
int tg_selftest_narrowphase(int32_t n_cases, int32_t n_hull, const double* hulls, const double* half, double* out);
/* The same for two hulls (csrc/tg_spin.hip's pair; oracle/narrowphase.c: mb_gjk_epa_hull_hull): hulls [n_cases][n_hull][3] = body A's hull in body
 * B's frame, hull_b [n_b][3] = body B's in its own frame (n_b <= 256); out as above. */
int tg_selftest_narrowphase_hulls(int32_t n_cases, int32_t n_hull, const double* hulls, int32_t n_b, const double* hull_b, double* out);
/* Self-test of the persistent manifold of csrc/tg_narrowphase.hpp (manifold_add / manifold_refresh; oracle/narrowphase.c: mb_manifold_add /
 * mb_manifold_refresh) under scripts of operations, one wavefront per case, the manifold in LDS and empty at the start.
 * ops [n_cases][n_ops][36] = kind (0 add, 1 refresh, anything else: nothing), breaking, oa[3], Ra[9] (row-major), ob[3], Rb[9], pa_w[3],
 * pb_w[3], n_w[3], depth (the last ten are read by an add only); out [n_cases][n_ops][65] = the manifold after each operation:
 * la[4][3], lb[4][3], nrm[4][3], pa[4][3], pb[4][3], depth[4], count. */
int tg_selftest_manifold(int32_t n_cases, int32_t n_ops, const double* ops, double* out);

/* Self-test of the raster's depth division (tactile_sensor.py:239-294 reads an IEEE depth buffer): n pseudo-random operand pairs
 * with exponents 2^-40 .. 2^24 divided by the kernels' refinement and by the correctly rounded `/`; *mismatches = quotients whose
 * bits differ (must be 0). */
int tg_selftest_division(int64_t n, uint64_t seed, int64_t* mismatches);
/* The same refinement where t_s_camera divides the clipped penetration by max_penetration = 0.05 (tactile_sensor.py:284-289): EVERY float in
 * {0} u [1e-4, 0.05] divided by 0.05f both ways; *mismatches must be 0. */
int tg_selftest_penetration_division(int64_t* mismatches);
/* Self-test of the raster's edge-function block test (csrc/tg_raster.hip: edges_exclude_rect - a record is skipped for a block of pixels that
 * its triangle provably cannot cover): n pseudo-random triangles (image-sized, slivers, huge, on pixel centres, heightfield-sized) x
 * rectangles as the kernels pass them, every pixel centre put through the pixel loops' own edge expressions.  out[0] = rectangles
 * excluded although they hold a coverable pixel (must be 0), out[1] = rectangles excluded, out[2] = rectangles without a coverable pixel.
 * The converse rule of round 5 (edges_cover_rect: a block wholly inside the triangle needs no coverage test per pixel): out[3] = rectangles
 * called covered in which some pixel fails the pixel loops' coverage predicate (must be 0), out[4] = rectangles called covered, out[5] =
 * rectangles whose every pixel passes.  out: int64 [6]. */
int tg_selftest_edge_exclusion(int64_t n, uint64_t seed, int64_t* out);

/* The block raster's hit predicate (csrc/tg_raster_dev.hpp: pixel_hit - a median for the bounding box, min3 / max3 for the signs of the edge
 * functions, s != 0 left to the NaN that the division then returns) against the chained compares of the other pixel loops, on the device,
 * from the pixel loop's own e0..e2, s and d.  n cases of one record and one quad of four pixel centres: half random (image-sized triangles,
 * slivers, coordinates up to 1e4, vertices on pixel centres), half forced specials (zero-area triangles in front of z, e_k = +-0, the
 * bounding box's edge on the pixel centre, +-inf and NaN coordinates).  out[0] = pixels whose (hit, new z) differ (must be 0), out[1] =
 * pixels hit, out[2] = pixels where the two forms' coverage booleans differ before the depth test (d is NaN there, or it counts in
 * out[0]), out[3] = pixels of forced specials.  out: int64 [4]. */
int tg_selftest_pixel_predicate(int64_t n, uint64_t seed, int64_t* out);

/* The tactile render (tg_render_tactile / tg_render_tactile_heightfield) with a chosen raster kernel.  TG_RK_AUTO = the product's choice
 * (csrc/tg_raster.hip: choose_render_kernel); any other id is launched if it can draw the input and refused (-1, nothing launched) if not:
 * the block kernel above 32 triangles, 128-wide tiles on a 64-wide image, a heightfield kernel for a mesh, and so on. */
enum {
    TG_RK_AUTO = 0,
    TG_RK_BLOCKS = 1,           /* k_render_blocks<16>: meshes of <= 32 triangles, 128-multiple images */
    TG_RK_SMALL_QREJ = 2,       /* k_render_small<128,64,2,true>: meshes of <= 256 triangles, with the per-quad reject */
    TG_RK_SMALL = 3,            /* k_render_small<128,64,2,false>: the same without it (every shared mesh of the product) */
    TG_RK_HF_BANDS = 4,         /* k_render_tactile<128,64,true>: heightfields, bounding-box band masks */
    TG_RK_HF_CELLS = 5,         /* k_render_tactile<128,64,true,true>: heightfields, edge-function cell masks */
    TG_RK_TACTILE_128 = 6,      /* k_render_tactile<128,128,false>: 128-multiple images */
    TG_RK_TACTILE_64 = 7,       /* k_render_tactile<64,64,false>: 64-multiple images */
    TG_RK_SCATTER_128 = 8,      /* k_render_scatter<128,128>: meshes, 128-multiple images */
    TG_RK_SCATTER_64 = 9        /* k_render_scatter<64,64>: meshes, 64-multiple images */
};
/* The kernel launch_render would launch (*chosen; -1: the forced one cannot draw the input) for a mesh, or (mesh NULL) a rows x cols
 * heightfield of spacing grid_scale, with the stimulus flags skip_quad_reject / fills_view / backface_cull (Stimulus::closed_outward; -1 when
 * asked for a mesh that is not closed and outward).  Host only: needs no device. */
int tg_selftest_render_kernel(const tg_sensor* sensor, const tg_mesh* mesh, int32_t rows, int32_t cols, double grid_scale, int32_t kernel,
                              int32_t skip_quad_reject, int32_t fills_view, int32_t backface_cull, int32_t* chosen);
/* Draws n images (1..65535) as the above with kernel `kernel`; *launched = the kernel launched.  heights [n][rows*cols], zoff [n]: the
 * heightfield when mesh is NULL.  out [n][H][W] is in / out: an env whose mask byte is 0 (mask NULL: all drawn) keeps what it held.
 * term_xf [n][12], term_mask [n], term_out [n][H][W] (all or none): the fused auto-reset's terminal layer - envs flagged in term_mask (and
 * in mask) also get the image of term_xf in term_out, the others keep what term_out held. */
int tg_selftest_render(const tg_sensor* sensor, const tg_mesh* mesh, int32_t rows, int32_t cols, double grid_scale, const double* heights,
                       const float* zoff, int32_t n, const float* xf, int32_t kernel, int32_t skip_quad_reject, int32_t fills_view,
                       int32_t backface_cull, const uint8_t* mask, const float* term_xf, const uint8_t* term_mask, uint8_t* term_out,
                       uint8_t* out, int32_t* launched);
/* tg_selftest_render followed (xf2 not NULL) by a second launch on the same image buffer and the same block tables, as a step after a step:
 * xf2 [n][12], mask2 [n] or NULL, and prev [n][H][W] (in / out) as the launch's save_prev - an env drawn by the second launch leaves the image
 * it held in prev, the others keep what prev held.  The terminal layer belongs to the first launch only. */
int tg_selftest_render_twice(const tg_sensor* sensor, const tg_mesh* mesh, int32_t rows, int32_t cols, double grid_scale, const double* heights,
                             const float* zoff, int32_t n, const float* xf, int32_t kernel, int32_t skip_quad_reject, int32_t fills_view,
                             int32_t backface_cull, const uint8_t* mask, const float* term_xf, const uint8_t* term_mask, uint8_t* term_out,
                             uint8_t* out, int32_t* launched, const float* xf2, const uint8_t* mask2, uint8_t* prev);
/* How tg_random_translate / tg_random_translate_rows would launch a call (csrc/tg_augment.h: translate_plan, the function the launcher itself
 * calls): in_dtype TG_AUGMENT_*, the layout, C, H, W, B and the addresses of the input and the output.  *path = 0 per element / 1 staged
 * through LDS, *chunks = 4096-element chunks per plane, *lds_bytes = dynamic LDS of a workgroup, *launches = kernel launches (B samples at
 * 2^23 workgroups per launch).  -1 for a shape the call itself refuses.  Host only: needs no device. */
int tg_selftest_translate_plan(int32_t in_dtype, int32_t channels_first, int32_t C, int32_t H, int32_t W, int64_t B, uint64_t in_addr,
                               uint64_t out_addr, int32_t* path, int32_t* chunks, int32_t* lds_bytes, int64_t* launches);
/* How tg_random_affine / tg_random_affine_rows would launch a call (csrc/tg_affine.h: affine_plan, the function the launcher itself calls):
 * *path = 0 per element / 1 taps gathered from global memory, float4 stores / 2 source rows staged through LDS; *in_vec = 1 when samples that
 * are not applied are copied with 16-byte loads; *chunks = 4096-element chunks per plane, *lds_bytes = dynamic LDS of a workgroup, *launches =
 * kernel launches.  -1 for a shape the call itself refuses.  Host only: needs no device. */
int tg_selftest_affine_plan(int32_t in_dtype, int32_t channels_first, int32_t C, int32_t H, int32_t W, int64_t B, uint64_t in_addr,
                            uint64_t out_addr, int32_t* path, int32_t* in_vec, int32_t* chunks, int32_t* lds_bytes, int64_t* launches);
/* The scene camera (csrc/tg_scene.hip: k_scene; the product reaches it through tg_set_scene / tg_render_scene) on any triangle set.
 * tg_selftest_scene_plan - host only, needs no device - runs the product's build_scene_chunks and scene_layout on verts [n_verts][3], tris
 * [n_tris][3], tri_frame [n_tris] (< 16), tri_rgb [n_tris][3] for a W x H image and reports *plan; the arrays (each may be NULL) receive
 * chunk_sphere [n_chunks][4] = centre, radius; chunk_table [n_chunks][5] = start, count, frame, vstart, vcount; cverts [n_cverts][3] the
 * chunk-ordered vertex copies; tris_out [n_tris][3] re-indexed into cverts; tri_local [n_tris] = i0 | i1 << 8 | i2 << 16 relative to vstart;
 * attr [n_tris] = frame << 24 | r << 16 | g << 8 | b, all in the chunk order.  Size them for n_chunks <= n_tris, n_cverts <= 3 n_tris. */
typedef struct tg_scene_plan {
    int32_t n_chunks, n_cverts;
    int32_t tile_w, tile_h, big_cap, lds_bytes;   /* the launch: tile, capacity of the LDS queue of large triangles, dynamic LDS bytes */
    int32_t accepted;                              /* 1: scene_prepare takes the scene, 0: it refuses it (too many chunks for the LDS) */
    int32_t small_area, big_area, huge_area, huge_cap, big_cap_max, chunk, max_chunks, max_spheres, max_frames;   /* kSmallArea ... kMaxFrames */
} tg_scene_plan;
int tg_selftest_scene_plan(int32_t n_verts, const float* verts, int32_t n_tris, const int32_t* tris, const uint8_t* tri_frame, const uint8_t* tri_rgb,
                           int32_t W, int32_t H, tg_scene_plan* plan, float* chunk_sphere, int32_t* chunk_table, float* cverts, int32_t* tris_out,
                           uint32_t* tri_local, uint32_t* attr);
/* Draws n images (1..65535) along the product's path: build_scene_chunks, scene_prepare, launch_scene_static when use_static, launch_scene.
 * The caller gives eye space: xf [n][n_frames][12] are the eye <- frame transforms themselves (R row-major, t) and light_eye the unit vector
 * towards the light.  THE FRAMES ARE RIGID OR UNIFORMLY SCALED - the kernel's own contract: its chunk cull takes the scale from the norm of one
 * matrix column.  With use_static the triangles of frame 0 are drawn once from env 0's xf [0] (the product's world frame: the same in every env).
 * Heightfield (hf_heights NULL: none): drawn in frame n_frames - 1 with hf_rgb; hf_sel NULL: hf_heights [n][rows * cols], hf_zoff [n]; else
 * hf_heights [3][n][rows * cols], hf_zoff [3][n], hf_sel [n] names each env's third (0..2).  spheres [n][n_spheres][8] (n_spheres <= 16) =
 * centre in eye space, radius, r, g, b (0..255), alpha (0: slot unused).  out [n][H][W][3] is in / out: an env whose mask byte is 0 (mask NULL:
 * all drawn) keeps what it held; prev (NULL or [n][H][W][3], in / out) is passed as save_prev: a drawn env's previous image goes there first.
 * Refused with -1, nothing launched, as tg_set_scene refuses: a side above 128 that is no multiple of 128, a bad projection, more than 16
 * frames or spheres, an index out of range, a scene that scene_prepare rejects; and n outside 1..65535.  The checks restate tg_set_scene's
 * (which reads them off a context) with one difference: an empty triangle set (n_tris == 0), which tg_set_scene refuses as an empty scene,
 * is drawn here - a heightfield or spheres alone. */
typedef struct tg_scene_test {
    int32_t image_h, image_w, n_verts, n_tris;
    const float* verts; const int32_t* tris; const uint8_t* tri_frame; const uint8_t* tri_rgb;
    int32_t n_frames, use_static;
    double fov_deg, near_plane, far_plane;
    float light_eye[3];
    uint8_t background[3], hf_rgb[3];
    const double* hf_heights; const float* hf_zoff; const uint8_t* hf_sel;
    int32_t hf_rows, hf_cols;
    double hf_scale;
    const float* spheres;
    int32_t n_spheres;
} tg_scene_test;
int tg_selftest_scene(const tg_scene_test* scene, int32_t n, const float* xf, const uint8_t* mask, uint8_t* out, uint8_t* prev);
/* The device frame stack (csrc/tg_stack.hip: launch_frame_stack / k_frame_stack, launch_obs_stack / k_obs_stack; the product reaches them
 * through tg_set_frame_stack / tg_set_obs_layout) on raw DEVICE buffers of the caller's (csrc/tg_stack_test.hip).  The fields are those of
 * StackArgs / StackVec / VisStack (csrc/tg_stack.h: layouts, modes and rules there); `which` names the launcher, and channels_first and the
 * vis_ block are read by TG_STACK_TEST_OBS only.  The launch goes on `stream`, unsynchronised.  Returns the launcher's own value: 0, -1 for
 * arguments it refuses (nothing launched), -2 when the launch failed.  Nothing is checked or allocated here. */
enum { TG_STACK_TEST_FRAME = 0, TG_STACK_TEST_OBS = 1 };
typedef struct tg_stack_test_vec {
    const float* src; const float* term; float* stack; float* term_stack;
    int32_t dim, pitch;
} tg_stack_test_vec;
typedef struct tg_stack_test {
    int32_t which, num_envs, n, mode, rewrite_all, channels_first;   /* mode: 0 step, 1 reset */
    int32_t H, W;
    const uint8_t* frame; const uint8_t* term_frame; const uint8_t* tmpl; uint8_t* stack; uint8_t* term_stack; uint8_t* rec;
    tg_stack_test_vec vec[2];
    const uint8_t* vis_frame; const uint8_t* vis_term_frame; uint8_t* vis_stack; uint8_t* vis_term_stack;
    int32_t vis_H, vis_W;
    const uint8_t* flag;
} tg_stack_test;
int tg_selftest_stack(const tg_stack_test* t, void* stream);
/* The device helpers of csrc/tg_physics.hpp (and rot_error of csrc/tg_kernels.hpp) one by one (csrc/tg_physics_test.hip), for T = double
 * (dtype 0) or float (dtype 1).  Case i is in [i][in_w], converted to T in the kernel, and runs in lane i % 64 of the one-wavefront workgroup
 * i / 64: THE CALLER DECIDES WHICH CASES SHARE A WAVEFRONT, and with it the outcome of the helpers' __any / __all votes; n is a multiple of 64
 * (pad with copies of a case: no idle lane votes).  out [i][out_w]; an integer result is the last column.  Quaternions x, y, z, w; matrices
 * row-major.  op: in -> out
 *    0 quat_from_euler  r, p, y -> q            1 euler_from_quat  q -> r, p, y        2 mat_from_quat  q -> R[9]       3 quat_from_mat  R[9] -> q
 *    4 quat_mul  a, b -> q                      5 axis_angle  axis[3], angle -> R[9]   6 rot_error  Rt[9], R[9] -> e[3] 7 plane_space  n[3] -> t1[3], t2[3]
 *    8 trsqrt  x -> y      9 trcp  x -> y      10 tsqrt_fast  x -> y                  11 inverse(S3)  xx, xy, xz, yy, yz, zz -> the same of the inverse
 *   12 friction_clamp  s1, s2, limit, cone (0: pyramid) -> s1, s2                      13 sincos_small  x -> sin, cos
 *   14 trig_init + k x (q += dq; trig_advance), N = 6:  k (0..24), q[6], dq[24][6] -> s[6], c[6], q[6]
 *   15 k x integrate_rotation:  k (0..240), R[9], w[3], dt -> R[9]
 *   16 solve_pivoted<T,6>  A[6][6], b[6] -> x[6]       17 solve_pivoted<T,8>  A[8][8], b[8] -> x[8]       18 pinv_apply<T,8>  J[6][8], b[6] -> x[8]
 *   19 pgs_unclamped  20 pgs_unclamped_blocks  21 pgs_clamped  22 pgs_threshold, N = 6;  23 - 26 the same, N = 8:
 *      Minv[N][N], rimp[N], jdi[N], iters, maximp, res_thr -> dv[N], the function's integer result (pgs_clamped: 0)
 * The loop counts (k, iters) stand around a wave vote and must be equal in the 64 lanes of a wavefront.  -1, nothing launched: unknown op or
 * dtype, a NULL pointer, n no positive multiple of 64, widths other than the op's, a loop count that is out of range or differs inside a
 * wavefront. */
int tg_selftest_physics(int32_t op, int32_t dtype, int32_t n, int32_t in_w, const double* in, int32_t out_w, double* out);
/* Writes arm and free-object states into a context of the product library (csrc/tg_state_test.hip), so that a test can start the step kernels
 * of object_push / object_roll / object_balance anywhere and not only at the reset pose (the product's own joint-state setter refuses envs with
 * a free object).  Every pointer is optional; the arrays are AoS [num_envs][k] doubles: mask [n] bytes (NULL: every env; an env whose byte is
 * 0 keeps all it holds), q, qd [n][ndof], body_pos [3], body_rot [9] row-major, body_linvel [3], body_angvel [3] (the cube, the marble, the
 * pole / round plate, the spinning plate's spool), ball_pos, ball_linvel, ball_angvel [3] (ball_on_plate), dish_state [18] = position,
 * rotation, linear and angular velocity (spinning_plate), goal_id [n] int32 (object_push, 0 .. traj_n_points; traj_n_points = past the last).
 * For the masked envs the given fields are transposed into the context's SoA state and what a teleport clears is cleared: the solver licence,
 * the pending one-shot force / torque of the last reset (with the ball's torque), the count of the cached contact manifold (tip - cube, dish -
 * spool), the contact pairs of the last tick.  The RNG, step count, trajectory, mass / radius, embed distance, gravity and episode return stay.
 * The context's stream is synchronised; nothing is rendered and no observation refreshed - the next step recomputes all it reports from the
 * state.  -1 and NOTHING WRITTEN: a NULL argument, a field the env kind does not have, a non-finite value, a rotation further than 1e-9 from
 * orthonormal (or with a negative determinant), a goal_id out of range.  -2: a HIP call failed. */
typedef struct tg_body_state_test {
    const uint8_t* mask;
    const double *q, *qd;
    const double *body_pos, *body_rot, *body_linvel, *body_angvel;
    const double *ball_pos, *ball_linvel, *ball_angvel;
    const double* dish_state;
    const int32_t* goal_id;
} tg_body_state_test;
int tg_selftest_set_body_state(tg_ctx* ctx, const tg_body_state_test* state);
/* Reads back the reset template of a context (State.reset_tmpl; csrc/tg_state_test.hip): the arm's post-reset state that the reset kernels
 * keep from the first move that ran through.  The context's stream is synchronised first.  *n_words = the template's size in doubles; out
 * [cap] receives them.  With N = the arm's joints: [0, N) q, [N, 2N) qd, [2N] reset ticks, [2N + 1] valid (0: not published yet), and in
 * object_push [2N + 2] path points, [2N + 3] the tip sphere's radius, [2N + 4 + 3k] the sphere's centre before tick k and, last, at the
 * final pose.  -1: a NULL argument, a context without a template (*n_words = 0), cap < *n_words.  -2: a HIP call failed. */
int tg_selftest_get_reset_template(tg_ctx* ctx, double* out, int32_t cap, int32_t* n_words);
/* The message of the last failing call of this library on the calling thread. */
const char* tg_selftest_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
