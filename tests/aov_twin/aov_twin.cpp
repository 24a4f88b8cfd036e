// AOV TWIN -- TEST INFRASTRUCTURE ONLY.
// The per-sample function of the first-hit feature planes (pathtracer-rs_amd/csrc/pt_aov.h: aov_item, the function k_aov runs per
// path) compiled for the CPU, behind the steps that feed it on the device: the scene as build_host_scene lays it out, camera_ray, the
// closest hit of bvh_trace (as the host twin's twin_trace_rays finds it).  One row of p_film in, the 12 floats of ptrs_render_aov's
// sample_aov out.  Never loaded by the product.
#include <string>

#include "../../pathtracer-rs_amd/csrc/pt_aov.h"

using namespace pt;

namespace { thread_local std::string g_err; }

extern "C" {

const char *aov_twin_last_error(void) { return g_err.c_str(); }

int aov_twin_rows(const PtrsSceneDesc *desc, const PtrsCamera *cam, float diff_scale, uint32_t n, const float *pfilm, float *out) {
    if (!desc || !cam || (n && (!pfilm || !out))) { g_err = "null argument"; return PTRS_ERR_INVALID; }
    HostScene H;
    int rc = build_host_scene(*desc, H, g_err);
    if (rc != PTRS_OK) return rc;
    const DScene sc = host_scene_view(H);
    const DCamera C = make_camera(*cam);
    DParams R;
    std::memset(&R, 0, sizeof(R));
    R.inv_sqrt_spp = diff_scale;
    for (uint32_t i = 0; i < n; ++i) {
        const f2 pf = mk2(pfilm[2 * (size_t)i], pfilm[2 * (size_t)i + 1]);
        const CamRay r = camera_ray(C, pf, diff_scale);
        LocalStack stk; HitRec h; uint32_t nn = 0, nt = 0;
        bvh_trace<false>(sc, r.o, r.d, PT_INF, stk, h, nn, nt);
        u4 hit; hit.x = hit_pack(h.prim, h.flags); hit.y = f2u(h.b0); hit.z = f2u(h.b1); hit.w = f2u(h.b2);
        aov_sample_row(aov_item<FEAT_FULL>(R, C, sc, pf, hit), out + (size_t)i * AOV_SAMPLE_FLOATS);
    }
    return PTRS_OK;
}

} // extern "C"
