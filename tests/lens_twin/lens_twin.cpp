// LENS TWIN -- TEST INFRASTRUCTURE ONLY.
// The thin-lens ray of the camera (pathtracer-rs_amd/csrc/pt_items.h: lens_ray, the function generate_item runs per path under
// PTRS_FLAG_THIN_LENS) compiled for the CPU behind make_camera, one row of (p_film, u_lens) in, o, d, rx_d, ry_d out -- for the
// float64 comparison of tests/test_thin_lens.py.  A lens of radius 0 gives camera_ray, as generate_item does.  lens_twin_aov_rows is
// tests/aov_twin's chain under the lens: that ray, bvh_trace's closest hit, aov_item WITH the generated ray (the form k_aov calls).
// Never loaded by the product.
#include <string>

#include "../../pathtracer-rs_amd/csrc/pt_aov.h"

using namespace pt;

extern "C" {

int lens_twin_rays(const PtrsCameraLens *cam, float diff_scale, uint32_t n, const float *pfilm, const float *ulens, float *out) {
    if (!cam || (n && (!pfilm || !ulens || !out))) return PTRS_ERR_INVALID;
    if (lens_error(cam->lens_radius, cam->focal_distance)) return PTRS_ERR_INVALID;
    const DCamera C = make_camera(cam->camera, PTRS_FLAG_THIN_LENS);
    for (uint32_t i = 0; i < n; ++i) {
        const f2 pf = mk2(pfilm[2 * (size_t)i], pfilm[2 * (size_t)i + 1]), ul = mk2(ulens[2 * (size_t)i], ulens[2 * (size_t)i + 1]);
        const CamRay r = C.lens_radius > 0.0f ? lens_ray(C, pf, ul, diff_scale) : camera_ray(C, pf, diff_scale);
        const f3 v[4] = {r.o, r.d, r.rx_d, r.ry_d};
        for (int k = 0; k < 4; ++k) { out[12 * (size_t)i + 3 * k] = v[k].x; out[12 * (size_t)i + 3 * k + 1] = v[k].y; out[12 * (size_t)i + 3 * k + 2] = v[k].z; }
    }
    return PTRS_OK;
}

int lens_twin_aov_rows(const PtrsSceneDesc *desc, const PtrsCameraLens *cam, float diff_scale, uint32_t n, const float *pfilm, const float *ulens, float *out) {
    if (!desc || !cam || (n && (!pfilm || !ulens || !out))) return PTRS_ERR_INVALID;
    if (lens_error(cam->lens_radius, cam->focal_distance)) return PTRS_ERR_INVALID;
    HostScene H;
    std::string err;
    int rc = build_host_scene(*desc, H, err);
    if (rc != PTRS_OK) return rc;
    const DScene sc = host_scene_view(H);
    const DCamera C = make_camera(cam->camera, PTRS_FLAG_THIN_LENS);
    DParams R;
    std::memset(&R, 0, sizeof(R));
    R.inv_sqrt_spp = diff_scale;
    for (uint32_t i = 0; i < n; ++i) {
        const f2 pf = mk2(pfilm[2 * (size_t)i], pfilm[2 * (size_t)i + 1]), ul = mk2(ulens[2 * (size_t)i], ulens[2 * (size_t)i + 1]);
        const CamRay r = C.lens_radius > 0.0f ? lens_ray(C, pf, ul, diff_scale) : camera_ray(C, pf, diff_scale);
        LocalStack stk; HitRec h; uint32_t nn = 0, nt = 0;
        bvh_trace<false>(sc, r.o, r.d, PT_INF, stk, h, nn, nt);
        u4 hit; hit.x = hit_pack(h.prim, h.flags); hit.y = f2u(h.b0); hit.z = f2u(h.b1); hit.w = f2u(h.b2);
        const f3 ray[2] = {r.o, r.d};
        aov_sample_row(aov_item<FEAT_FULL>(R, C, sc, pf, hit, ray), out + (size_t)i * AOV_SAMPLE_FLOATS);
    }
    return PTRS_OK;
}

} // extern "C"
