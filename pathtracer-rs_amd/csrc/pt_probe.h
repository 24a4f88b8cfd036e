// pt_probe.h -- per-row probes of one material's BSDF and of one light, for known-answer tests only.
//
// The render kernels never include this file.  The gfx950 test entry points (ptrs_probe_bsdf /
// ptrs_probe_light) and the host twin run exactly these functions, so a test can evaluate the
// device code's f / pdf / sample_f and sample_li / pdf_li / le at directions and random numbers of
// its choosing -- grazing, on the normal, subnormal, at the ends of [0,1) -- instead of where renders
// happen to go.
#pragma once
#include "pt_light.h"

namespace pt {

enum : uint32_t { PROBE_BSDF_IN = 8, PROBE_BSDF_OUT = 16, PROBE_LIGHT_IN = 5, PROBE_LIGHT_OUT = 16 };

// A synthetic hit for a BSDF probe: geometric normal ng, shading normal ns, shading dpdu (the
// bsdf's ss = normalize(dpdu), ts = ns x ss: the caller passes dpdu orthogonal to ns).
PT_HD Surface probe_surface(const float *frame /* ng, ns, dpdu */, f3 wo) {
    Surface s;
    s.p = splat3(0.0f); s.p_error = splat3(0.0f); s.wo = wo;
    s.n = mk3(frame[0], frame[1], frame[2]);
    s.ns = mk3(frame[3], frame[4], frame[5]);
    s.dpdu = mk3(frame[6], frame[7], frame[8]); s.dpdv = cross(s.ns, s.dpdu);
    s.s_dpdu = s.dpdu; s.s_dpdv = s.dpdv;
    s.uv = mk2(0.25f, 0.5f);
    s.dudx = s.dvdx = s.dudy = s.dvdy = 0.0f;
    s.prim = 0; s.ssn = s.dpdu; s.ssn_ok = false;
    return s;
}

// in: wo.xyz, wi.xyz, u.xy (world space).  out: bsdf_f(wo, wi).rgb, bsdf_pdf(wo, wi), sample_f(wo, u): f.rgb, pdf, wi.xyz
// (0 when nothing was sampled), sampled flags, then 1 when the material yields a BSDF (0: Q17), 0, 0, 0.
template <int MAT>
PT_HD void bsdf_probe_mat(const DScene &sc, int32_t mat_id, const float *frame, const float *in, float *out) {
    const f3 wo = mk3(in[0], in[1], in[2]), wi = mk3(in[3], in[4], in[5]);
    const f2 u = mk2(in[6], in[7]);
    Surface s = probe_surface(frame, wo);
    BsdfT<MatLobes<MAT>::N> b;
    for (uint32_t k = 0; k < PROBE_BSDF_OUT; ++k) out[k] = 0.0f;
    if (!make_bsdf<MAT, 0>(sc, mat_id, s, b)) return;
    const f3 f = bsdf_f(b, wo, wi, BSDF_ALL);
    const float pdf = bsdf_pdf(b, wo, wi, BSDF_ALL);
    f3 swi = splat3(0.0f); float spdf = 0.0f; uint32_t sampled = 0;
    const f3 sf = bsdf_sample_f(b, wo, swi, u, spdf, BSDF_ALL, sampled);
    out[0] = f.x; out[1] = f.y; out[2] = f.z; out[3] = pdf;
    out[4] = sf.x; out[5] = sf.y; out[6] = sf.z; out[7] = spdf;
    out[8] = swi.x; out[9] = swi.y; out[10] = swi.z; out[11] = (float)sampled;
    out[12] = 1.0f;
}

// kind: the material's kind (0 Matte, 1 Metal, 2 Mirror, 3 Glass, 4 Disney, 5 Substrate); the caller has checked it
PT_HD void bsdf_probe_row(const DScene &sc, int32_t mat_id, int32_t kind, const float *frame, const float *in, float *out) {
    switch (kind) {
        case 0: bsdf_probe_mat<0>(sc, mat_id, frame, in, out); break;
        case 1: bsdf_probe_mat<1>(sc, mat_id, frame, in, out); break;
        case 2: bsdf_probe_mat<2>(sc, mat_id, frame, in, out); break;
        case 3: bsdf_probe_mat<3>(sc, mat_id, frame, in, out); break;
        case 4: bsdf_probe_mat<4>(sc, mat_id, frame, in, out); break;
        default: bsdf_probe_mat<5>(sc, mat_id, frame, in, out); break;
    }
}

// One light of kind 2 (triangle) or 3 (environment) seen from the reference point p with normal n (p_error 0).
// in: u.xy, w_query.xyz.  out: sample_li(u): wi.xyz, pdf, Li.rgb, ok; pdf_li(w_query); le(w_query).rgb; 0, 0, 0, 0.
PT_HD void light_probe_row(const DScene &sc, int32_t light, const float *ref /* p, n */, const float *in, float *out) {
    const DLight &L = sc.lights[light];
    const f3 p = mk3(ref[0], ref[1], ref[2]), n = mk3(ref[3], ref[4], ref[5]);
    const SpawnPair sp = spawn_pair(p, splat3(0.0f), n);
    const f3 wq = mk3(in[2], in[3], in[4]);
    LightSample ls;
    const bool ok = light_sample_li<FEAT_IMG_ENV>(sc, L, p, sp, mk2(in[0], in[1]), ls);
    const float pq = light_pdf_li<FEAT_IMG_ENV>(sc, L, p, sp, wq);
    const f3 le = light_le<FEAT_IMG_ENV>(sc, L, wq);
    for (uint32_t k = 0; k < PROBE_LIGHT_OUT; ++k) out[k] = 0.0f;
    out[0] = ls.wi.x; out[1] = ls.wi.y; out[2] = ls.wi.z; out[3] = ls.pdf;
    out[4] = ls.li.x; out[5] = ls.li.y; out[6] = ls.li.z; out[7] = ok ? 1.0f : 0.0f;
    out[8] = pq; out[9] = le.x; out[10] = le.y; out[11] = le.z;
}

} // namespace pt
