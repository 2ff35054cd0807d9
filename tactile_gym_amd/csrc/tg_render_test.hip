// tg_render_test.hip - libtactile_gym_hip_test.so: the tactile render with a chosen kernel (tg_selftest_render) and launch_render's choice
// without a device (tg_selftest_render_kernel).  TEST INFRASTRUCTURE (include/tactile_gym_hip_test.h): linked with the product's own raster
// object (tg_raster.o), so the kernels under test are the product's; tests/test_gpu_raster_matrix.py and tests/test_raster_f64_cpu.py call it.
#include "../../include/tactile_gym_hip_test.h"
#include "tg_ctx.hpp"

namespace tg {

// The stimulus as tg_create / tg_render_tactile build it; soup / heights pointers are left null (choose_render_kernel reads none of them).
static int render_test_setup(const tg_sensor* sen, const tg_mesh* mesh, int32_t rows, int32_t cols, double grid_scale, int32_t kernel,
                             int32_t skip_quad_reject, int32_t fills_view, int32_t backface_cull, RasterParams* P, Stimulus* S) {
    if (!sen || !sen->nodef_dep || !sen->nodef_gray || !sen->border_mask) return fail(-1, "NULL sensor");
    const int H = sen->image_h, W = sen->image_w;
    if (H < 64 || W < 64 || H % 64 != 0 || W % 64 != 0) return fail(-1, "image sides must be multiples of 64");
    if (kernel < kRkAuto || kernel > kRkScatter64) return fail(-1, "unknown kernel id");
    *P = make_raster_params(W, H, sen->fov_deg, sen->near_plane, sen->far_plane, sen->turn_off_border, sen->nodef_dep);
    *S = Stimulus{};
    S->force_kernel = kernel;
    if (mesh) {
        if (mesh->n_tris < 0 || (mesh->n_tris > 0 && (!mesh->verts || !mesh->tris))) return fail(-1, "bad mesh");
        S->kind = 0; S->n_tris = mesh->n_tris;
        S->skip_quad_reject = skip_quad_reject ? 1 : 0;
        S->fills_view = fills_view ? 1 : 0;
        if (backface_cull && !mesh_closed_outward(mesh)) return fail(-1, "back-face cull asked for a mesh that is not closed and outward");
        S->closed_outward = backface_cull ? 1 : 0;
    } else {
        if (rows < 2 || cols < 2 || !(grid_scale > 0.0)) return fail(-1, "bad heightfield");
        S->kind = 1; S->rows = rows; S->cols = cols; S->scale = (float)grid_scale; S->n_tris = (rows - 1) * (cols - 1) * 2;
    }
    return 0;
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_selftest_render_kernel(const tg_sensor* sen, const tg_mesh* mesh, int32_t rows, int32_t cols, double grid_scale, int32_t kernel,
                              int32_t skip_quad_reject, int32_t fills_view, int32_t backface_cull, int32_t* chosen) {
    if (!chosen) return fail(-1, "NULL argument");
    RasterParams P; Stimulus S;
    if (int rc = render_test_setup(sen, mesh, rows, cols, grid_scale, kernel, skip_quad_reject, fills_view, backface_cull, &P, &S)) return rc;
    static const float dummy[1] = {0.0f};   // make_block_tables sets both tables for every 128-multiple image
    if (P.W % 128 == 0 && P.H % 128 == 0) { P.blockmax = dummy; P.tmpl = reinterpret_cast<const uint8_t*>(dummy); }
    *chosen = choose_render_kernel(P, S);
    return 0;
}

int tg_selftest_render_twice(const tg_sensor* sen, const tg_mesh* mesh, int32_t rows, int32_t cols, double grid_scale, const double* heights,
                             const float* zoff, int32_t n, const float* xf, int32_t kernel, int32_t skip_quad_reject, int32_t fills_view,
                             int32_t backface_cull, const uint8_t* mask, const float* term_xf, const uint8_t* term_mask, uint8_t* term_out,
                             uint8_t* out, int32_t* launched, const float* xf2, const uint8_t* mask2, uint8_t* prev) {
    if (!launched) return fail(-1, "NULL argument");
    if (xf2 && !prev) return fail(-1, "a second launch saves the first one's images: prev is needed");
    *launched = -1;
    if (!xf || !out) return fail(-1, "NULL argument");
    if (!mesh && (!heights || !zoff)) return fail(-1, "a mesh or a heightfield");
    if ((term_xf != nullptr) != (term_mask != nullptr) || (term_xf != nullptr) != (term_out != nullptr)) return fail(-1, "term_xf / term_mask / term_out: all or none");
    if (n < 1 || n > 65535) return fail(-1, "n must be in 1..65535 (the render launch carries the env index in grid.y)");
    RasterParams P; Stimulus S;
    if (int rc = render_test_setup(sen, mesh, rows, cols, grid_scale, kernel, skip_quad_reject, fills_view, backface_cull, &P, &S)) return rc;
    if (int rc = need_device()) return rc;
    const int H = sen->image_h, W = sen->image_w;
    const size_t npix = (size_t)H * W, cells = mesh ? 0 : (size_t)rows * cols;
    DevBuf nd, ng, bm, xx, oo, mk, tx, tm, to, hh, zz, sp, bt, x2, m2, pv;
    if (nd.alloc(npix * 4) || ng.alloc(npix) || bm.alloc(npix) || xx.alloc((size_t)n * 48) || oo.alloc(npix * n)) return fail(-2, "hipMalloc failed");
    TG_HIP(hipMemcpy(nd.p, sen->nodef_dep, npix * 4, hipMemcpyHostToDevice));
    { std::vector<uint8_t> g8(npix); make_gray_u8(sen->nodef_gray, (int)npix, g8.data()); TG_HIP(hipMemcpy(ng.p, g8.data(), npix, hipMemcpyHostToDevice)); }
    TG_HIP(hipMemcpy(bm.p, sen->border_mask, npix, hipMemcpyHostToDevice));
    TG_HIP(hipMemcpy(xx.p, xf, (size_t)n * 48, hipMemcpyHostToDevice));
    TG_HIP(hipMemcpy(oo.p, out, npix * n, hipMemcpyHostToDevice));          // what the caller put there: masked-out envs must keep it
    if (mask) {
        if (mk.alloc((size_t)n)) return fail(-2, "hipMalloc failed");
        TG_HIP(hipMemcpy(mk.p, mask, (size_t)n, hipMemcpyHostToDevice));
    }
    if (term_xf) {
        if (tx.alloc((size_t)n * 48) || tm.alloc((size_t)n) || to.alloc(npix * n)) return fail(-2, "hipMalloc failed");
        TG_HIP(hipMemcpy(tx.p, term_xf, (size_t)n * 48, hipMemcpyHostToDevice));
        TG_HIP(hipMemcpy(tm.p, term_mask, (size_t)n, hipMemcpyHostToDevice));
        TG_HIP(hipMemcpy(to.p, term_out, npix * n, hipMemcpyHostToDevice));
    }
    if (make_block_tables(P, sen->nodef_dep, sen->nodef_gray, sen->border_mask, n, &bt.p)) return fail(-2, "hipMalloc failed");
    if (mesh) {
        std::vector<float> soup((size_t)mesh->n_tris * 9);
        for (int t = 0; t < mesh->n_tris; ++t)
            for (int k = 0; k < 3; ++k) {
                const int v = mesh->tris[3 * t + k];
                if (v < 0 || v >= mesh->n_verts) return fail(-1, "triangle index out of range");
                for (int a = 0; a < 3; ++a) soup[(size_t)t * 9 + 3 * k + a] = mesh->verts[3 * (size_t)v + a];
            }
        if (sp.alloc(soup.size() * 4 + 4)) return fail(-2, "hipMalloc failed");
        TG_HIP(hipMemcpy(sp.p, soup.data(), soup.size() * 4, hipMemcpyHostToDevice));
        S.soup = (const float*)sp.p;
    } else {
        if (hh.alloc(cells * n * 8) || zz.alloc((size_t)n * 4)) return fail(-2, "hipMalloc failed");
        TG_HIP(hipMemcpy(hh.p, heights, cells * n * 8, hipMemcpyHostToDevice)); TG_HIP(hipMemcpy(zz.p, zoff, (size_t)n * 4, hipMemcpyHostToDevice));
        S.heights = (const double*)hh.p; S.zoff = (const float*)zz.p;
    }
    const int k = launch_render(P, S, (const float*)xx.p, 0, n, (const uint8_t*)mk.p, (const float*)nd.p, (const uint8_t*)ng.p, (const uint8_t*)bm.p,
                                (uint8_t*)oo.p, nullptr, (const float*)tx.p, (const uint8_t*)tm.p, (uint8_t*)to.p, 0);
    if (k < 0) return fail(-1, "the forced kernel cannot draw this input");
    TG_HIP(hipGetLastError());
    if (xf2) {   // the same image buffer and the same block tables (the changed-block record of the first launch), the old images saved
        if (x2.alloc((size_t)n * 48) || pv.alloc(npix * n) || (mask2 && m2.alloc((size_t)n))) return fail(-2, "hipMalloc failed");
        TG_HIP(hipMemcpy(x2.p, xf2, (size_t)n * 48, hipMemcpyHostToDevice));
        TG_HIP(hipMemcpy(pv.p, prev, npix * n, hipMemcpyHostToDevice));
        if (mask2) TG_HIP(hipMemcpy(m2.p, mask2, (size_t)n, hipMemcpyHostToDevice));
        if (launch_render(P, S, (const float*)x2.p, 0, n, (const uint8_t*)m2.p, (const float*)nd.p, (const uint8_t*)ng.p, (const uint8_t*)bm.p,
                          (uint8_t*)oo.p, (uint8_t*)pv.p, nullptr, nullptr, nullptr, 0) != k) return fail(-3, "the second launch chose another kernel");
        TG_HIP(hipGetLastError());
    }
    TG_HIP(hipDeviceSynchronize());
    if (xf2) TG_HIP(hipMemcpy(prev, pv.p, npix * n, hipMemcpyDeviceToHost));
    TG_HIP(hipMemcpy(out, oo.p, npix * n, hipMemcpyDeviceToHost));
    if (term_xf) TG_HIP(hipMemcpy(term_out, to.p, npix * n, hipMemcpyDeviceToHost));
    *launched = k;
    return 0;
}

int tg_selftest_render(const tg_sensor* sen, const tg_mesh* mesh, int32_t rows, int32_t cols, double grid_scale, const double* heights,
                       const float* zoff, int32_t n, const float* xf, int32_t kernel, int32_t skip_quad_reject, int32_t fills_view,
                       int32_t backface_cull, const uint8_t* mask, const float* term_xf, const uint8_t* term_mask, uint8_t* term_out,
                       uint8_t* out, int32_t* launched) {
    return tg_selftest_render_twice(sen, mesh, rows, cols, grid_scale, heights, zoff, n, xf, kernel, skip_quad_reject, fills_view, backface_cull,
                                    mask, term_xf, term_mask, term_out, out, launched, nullptr, nullptr, nullptr);
}

const char* tg_selftest_last_error(void) { return g_err.c_str(); }

}  // extern "C"
