/*
 * tactile_gym_hip_test.h - C ABI of libtactile_gym_hip_test.so: device self-tests of pieces of the product's kernels.
 *
 * TEST INFRASTRUCTURE, not part of the boundary a maintainer binds (that is tactile_gym_hip.h / libtactile_gym_hip.so): built by
 * csrc/build.sh next to the product library from the same device headers, loaded only by tests/ (tactile_gym_amd._capi.test_lib()).
 * Every function returns 0 on success, -1 bad argument, -2 no HIP device / allocation failed, -3 launch failed.
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
/* How tg_random_translate / tg_random_translate_rows would launch a call (csrc/tg_augment.h: translate_plan, the function the launcher itself
 * calls): in_dtype TG_AUGMENT_*, the layout, C, H, W, B and the addresses of the input and the output.  *path = 0 per element / 1 staged
 * through LDS, *chunks = 4096-element chunks per plane, *lds_bytes = dynamic LDS of a workgroup, *launches = kernel launches (B samples at
 * 2^23 workgroups per launch).  -1 for a shape the call itself refuses.  Host only: needs no device. */
int tg_selftest_translate_plan(int32_t in_dtype, int32_t channels_first, int32_t C, int32_t H, int32_t W, int64_t B, uint64_t in_addr,
                               uint64_t out_addr, int32_t* path, int32_t* chunks, int32_t* lds_bytes, int64_t* launches);
/* The message of the last failing call of this library on the calling thread. */
const char* tg_selftest_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
