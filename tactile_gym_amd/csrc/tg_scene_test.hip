// tg_scene_test.hip - libtactile_gym_hip_test.so: the scene camera on any triangle set (tg_selftest_scene) and its host-side plan - chunk
// table, LDS layout, constants - without a device (tg_selftest_scene_plan).  TEST INFRASTRUCTURE (include/tactile_gym_hip_test.h): linked with
// the product's own tg_scene.o, so build_scene_chunks, scene_layout, scene_prepare, the launches and k_scene are the product's;
// tests/test_scene_cases_cpu.py and tests/test_gpu_scene_matrix.py call it.
#include "../../include/tactile_gym_hip_test.h"
#include "tg_ctx.hpp"
#include "tg_scene.h"

namespace tg {

// The checks of tg_set_scene, in its order, and the attribute words it builds.
static int scene_test_attr(int32_t n_verts, const float* verts, int32_t n_tris, const int32_t* tris, const uint8_t* tri_frame, const uint8_t* tri_rgb,
                           int32_t W, int32_t H, int32_t n_frames, std::vector<uint32_t>& attr) {
    if (n_tris < 0 || n_verts < 0 || (n_tris > 0 && (!verts || !tris || !tri_frame || !tri_rgb || n_verts == 0))) return fail(-1, "bad triangle set");
    if (W <= 0 || H <= 0 || (W > 128 && W % 128) || (H > 128 && H % 128)) return fail(-1, "image sides must be <= 128 or multiples of 128");
    if (n_frames < 1 || n_frames > 16) return fail(-1, "n_frames must be in 1..16");
    attr.resize(n_tris);
    for (int t = 0; t < n_tris; ++t) {
        if (tri_frame[t] >= n_frames) return fail(-1, "tri_frame out of range");
        for (int k = 0; k < 3; ++k)
            if (tris[3 * t + k] < 0 || tris[3 * t + k] >= n_verts) return fail(-1, "vertex index out of range");
        attr[t] = ((uint32_t)tri_frame[t] << 24) | ((uint32_t)tri_rgb[3 * t] << 16) | ((uint32_t)tri_rgb[3 * t + 1] << 8) | tri_rgb[3 * t + 2];
    }
    return 0;
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_selftest_scene_plan(int32_t n_verts, const float* verts, int32_t n_tris, const int32_t* tris, const uint8_t* tri_frame, const uint8_t* tri_rgb,
                           int32_t W, int32_t H, tg_scene_plan* plan, float* chunk_sphere, int32_t* chunk_table, float* cverts_out, int32_t* tris_out,
                           uint32_t* tri_local_out, uint32_t* attr_out) {
    if (!plan) return fail(-1, "NULL argument");
    std::vector<uint32_t> attr;
    if (int rc = scene_test_attr(n_verts, verts, n_tris, tris, tri_frame, tri_rgb, W, H, 16, attr)) return rc;
    std::vector<int32_t> t2(tris, tris + (size_t)n_tris * 3);
    std::vector<SceneChunk> chunks;
    std::vector<float> cverts;
    std::vector<uint32_t> tri_local;
    build_scene_chunks(verts, t2.data(), attr.data(), n_tris, chunks, cverts, tri_local);
    const SceneLayout L = scene_layout(W, H, (int)chunks.size());
    plan->n_chunks = (int32_t)chunks.size(); plan->n_cverts = (int32_t)(cverts.size() / 3);
    plan->big_cap = L.big_cap; plan->lds_bytes = (int32_t)L.lds_bytes; plan->accepted = L.fits; plan->tile_w = L.tw; plan->tile_h = L.th;
    plan->small_area = L.small_area; plan->big_area = L.big_area; plan->huge_area = L.huge_area; plan->huge_cap = L.huge_cap;
    plan->big_cap_max = L.big_cap_max; plan->chunk = L.chunk; plan->max_chunks = L.max_chunks; plan->max_spheres = L.max_spheres;
    plan->max_frames = L.max_frames;
    for (size_t i = 0; i < chunks.size(); ++i) {
        const SceneChunk& c = chunks[i];
        if (chunk_sphere) { chunk_sphere[4 * i] = c.cx; chunk_sphere[4 * i + 1] = c.cy; chunk_sphere[4 * i + 2] = c.cz; chunk_sphere[4 * i + 3] = c.r; }
        if (chunk_table) { int32_t* r = chunk_table + 5 * i; r[0] = c.start; r[1] = c.count; r[2] = c.frame; r[3] = c.vstart; r[4] = c.vcount; }
    }
    if (cverts_out) std::copy(cverts.begin(), cverts.end(), cverts_out);
    if (tris_out) std::copy(t2.begin(), t2.end(), tris_out);
    if (tri_local_out) std::copy(tri_local.begin(), tri_local.end(), tri_local_out);
    if (attr_out) std::copy(attr.begin(), attr.end(), attr_out);
    return 0;
}

int tg_selftest_scene(const tg_scene_test* sc, int32_t n, const float* xf, const uint8_t* mask, uint8_t* out, uint8_t* prev) {
    if (!sc || !xf || !out) return fail(-1, "NULL argument");
    std::vector<uint32_t> attr;
    const int W = sc->image_w, H = sc->image_h, nf = sc->n_frames;
    if (int rc = scene_test_attr(sc->n_verts, sc->verts, sc->n_tris, sc->tris, sc->tri_frame, sc->tri_rgb, W, H, nf, attr)) return rc;
    if (!(sc->near_plane > 0 && sc->far_plane > sc->near_plane && sc->fov_deg > 0 && sc->fov_deg < 180)) return fail(-1, "bad projection");
    if (n < 1 || n > 65535) return fail(-1, "n must be in 1..65535 (the scene launch carries the env index in grid.y)");
    if (sc->n_spheres < 0 || sc->n_spheres > 16 || (sc->n_spheres > 0 && !sc->spheres)) return fail(-1, "0..16 spheres");
    const bool hf = sc->hf_heights != nullptr;
    if (hf && (!sc->hf_zoff || sc->hf_rows < 2 || sc->hf_cols < 2 || !(sc->hf_scale > 0.0))) return fail(-1, "bad heightfield");
    SceneParams P = make_scene_params(W, H, sc->fov_deg, sc->near_plane, sc->far_plane);
    for (int k = 0; k < 3; ++k) { P.light_eye[k] = sc->light_eye[k]; P.background[k] = sc->background[k]; }
    P.n_tris = sc->n_tris; P.n_frames = nf;
    std::vector<int32_t> tris(sc->tris, sc->tris + (size_t)sc->n_tris * 3);
    std::vector<SceneChunk> chunks;
    std::vector<float> cverts;
    std::vector<uint32_t> tri_local;
    build_scene_chunks(sc->verts, tris.data(), attr.data(), sc->n_tris, chunks, cverts, tri_local);
    P.n_chunks = (int)chunks.size();
    if (!scene_layout(W, H, P.n_chunks).fits) return fail(-1, "the scene's chunk list does not fit the workgroup's LDS");
    if (int rc = need_device()) return rc;
    const size_t img = (size_t)W * H * 3, nn = (size_t)n;
    DevBuf dch, dv, dt, dl, da, dx, dout, dprev, dmask, dst, dsp, dh, dz, dsel;
    if (dch.alloc(chunks.size() * sizeof(SceneChunk)) || dv.alloc(cverts.size() * 4 + 16) || dt.alloc(tris.size() * 4) || dl.alloc(tri_local.size() * 4) ||
        da.alloc(attr.size() * 4) || dx.alloc(nn * nf * 48) || dout.alloc(nn * img))
        return fail(-2, "hipMalloc failed");
    TG_HIP(hipMemcpy(dch.p, chunks.data(), chunks.size() * sizeof(SceneChunk), hipMemcpyHostToDevice));
    TG_HIP(hipMemcpy(dv.p, cverts.data(), cverts.size() * 4, hipMemcpyHostToDevice));
    TG_HIP(hipMemcpy(dt.p, tris.data(), tris.size() * 4, hipMemcpyHostToDevice));
    TG_HIP(hipMemcpy(dl.p, tri_local.data(), tri_local.size() * 4, hipMemcpyHostToDevice));
    TG_HIP(hipMemcpy(da.p, attr.data(), attr.size() * 4, hipMemcpyHostToDevice));
    TG_HIP(hipMemcpy(dx.p, xf, nn * nf * 48, hipMemcpyHostToDevice));
    TG_HIP(hipMemcpy(dout.p, out, nn * img, hipMemcpyHostToDevice));          // what the caller put there: masked-out envs must keep it
    P.chunks = (const SceneChunk*)dch.p; P.verts = (const float*)dv.p; P.tris = (const int32_t*)dt.p; P.tri_local = (const uint32_t*)dl.p;
    P.tri_attr = (const uint32_t*)da.p;
    if (mask) {
        if (dmask.alloc(nn)) return fail(-2, "hipMalloc failed");
        TG_HIP(hipMemcpy(dmask.p, mask, nn, hipMemcpyHostToDevice));
    }
    if (prev) {
        if (dprev.alloc(nn * img)) return fail(-2, "hipMalloc failed");
        TG_HIP(hipMemcpy(dprev.p, prev, nn * img, hipMemcpyHostToDevice));
    }
    if (sc->n_spheres > 0) {
        const size_t b = nn * sc->n_spheres * 32;
        if (dsp.alloc(b)) return fail(-2, "hipMalloc failed");
        TG_HIP(hipMemcpy(dsp.p, sc->spheres, b, hipMemcpyHostToDevice));
        P.spheres = (const float*)dsp.p; P.n_spheres = sc->n_spheres;
    }
    if (hf) {
        const size_t thirds = sc->hf_sel ? 3 : 1, cells = (size_t)sc->hf_rows * sc->hf_cols;
        if (dh.alloc(thirds * nn * cells * 8) || dz.alloc(thirds * nn * 4)) return fail(-2, "hipMalloc failed");
        TG_HIP(hipMemcpy(dh.p, sc->hf_heights, thirds * nn * cells * 8, hipMemcpyHostToDevice));
        TG_HIP(hipMemcpy(dz.p, sc->hf_zoff, thirds * nn * 4, hipMemcpyHostToDevice));
        if (sc->hf_sel) {
            if (dsel.alloc(nn)) return fail(-2, "hipMalloc failed");
            TG_HIP(hipMemcpy(dsel.p, sc->hf_sel, nn, hipMemcpyHostToDevice));
        }
        P.hf_heights = (const double*)dh.p; P.hf_zoff = (const float*)dz.p; P.hf_sel = (const uint8_t*)dsel.p; P.hf_n = n;
        P.hf_rows = sc->hf_rows; P.hf_cols = sc->hf_cols; P.hf_scale = (float)sc->hf_scale;
        P.hf_rgb = ((uint32_t)sc->hf_rgb[0] << 16) | ((uint32_t)sc->hf_rgb[1] << 8) | sc->hf_rgb[2];
    }
    if (scene_prepare(P) != 0) return fail(-1, "scene_prepare refused the scene (or hipFuncSetAttribute failed)");
    if (sc->use_static) {
        if (dst.alloc((size_t)W * H * 8)) return fail(-2, "hipMalloc failed");
        launch_scene_static(P, (const float*)dx.p, (unsigned long long*)dst.p, 0);
        TG_HIP(hipGetLastError());
        TG_HIP(hipDeviceSynchronize());
        P.static_keys = (const unsigned long long*)dst.p;
    }
    launch_scene(P, (const float*)dx.p, n, (const uint8_t*)dmask.p, (uint8_t*)dout.p, (uint8_t*)dprev.p, 0);
    TG_HIP(hipGetLastError());
    TG_HIP(hipDeviceSynchronize());
    TG_HIP(hipMemcpy(out, dout.p, nn * img, hipMemcpyDeviceToHost));
    if (prev) TG_HIP(hipMemcpy(prev, dprev.p, nn * img, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
