// pt_probe.h -- per-row probes of one material's BSDF, of one light, of one texture, of one triangle's hit surface and of the
// arithmetic substrate itself (include/ptrs_detmath.h, pt_vec.h), for known-answer tests only.
//
// The render kernels never include this file.  The gfx950 test entry points (ptrs_probe_bsdf /
// ptrs_probe_light) and the host twin run exactly these functions, so a test can evaluate the
// device code's f / pdf / sample_f and sample_li / pdf_li / le at directions and random numbers of
// its choosing -- grazing, on the normal, subnormal, at the ends of [0,1) -- instead of where renders
// happen to go.
#pragma once
#include "pt_light.h"
#include "pt_bvh.h"
#include "pt_host_scene.h"

namespace pt {

enum : uint32_t { PROBE_BSDF_IN = 8, PROBE_BSDF_OUT = 16, PROBE_LIGHT_IN = 5, PROBE_LIGHT_OUT = 16, PROBE_TEX_IN = 6, PROBE_TEX_OUT = 8,
                  PROBE_SURF_IN = 16, PROBE_SURF_OUT = 64, PROBE_MATH_IN = 16, PROBE_MATH_OUT = 16,
                  PROBE_SHADE_IN = 12, PROBE_SHADE_OUT = 12, PROBE_SHADE_HEADER = 12 /* 32-bit words: ptrs_probe_shade_tables (device only) */ };
enum : uint32_t { PROBE_SHADE_SOBOL = 0, PROBE_SHADE_ENV = 1, PROBE_SHADE_NUM_OPS };

// ptrs_probe_shade_tables' checks of its rows (no device needed): nullptr, or why the call is refused.  A Sobol' row draws N of 1, 2, 3
// or 8 dimensions below 1024 (the batch sizes shade_item draws; the tables end at 1024); an environment row samples an
// InfiniteAreaLight of the scene with u in [0, 1)^2.  H == nullptr: the checks that need no scene.
inline const char *probe_shade_rows_check(const HostScene *H, uint32_t op, uint32_t n, const uint32_t *rows) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t *r = rows + (size_t)i * PROBE_SHADE_IN;
        if (op == PROBE_SHADE_SOBOL) {
            const uint32_t N = r[3];
            if (N != 1u && N != 2u && N != 3u && N != 8u) return "a Sobol' row draws 1, 2, 3 or 8 dimensions";
            for (uint32_t k = 0; k < N; ++k) if (r[4 + k] >= 1024u) return "sobol sampler can only sample up to 1024 dimensions";
        } else {
            float u[2]; std::memcpy(u, r, 8);
            if (!(u[0] >= 0.0f && u[0] < 1.0f && u[1] >= 0.0f && u[1] < 1.0f)) return "u outside [0, 1)";
            if (H && ((size_t)r[2] >= H->lights.size() || H->lights[r[2]].kind != 3)) return "the row's light is not an environment light of the scene";
        }
    }
    return nullptr;
}

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

// Texture `tex` at one lookup.  in: uv.xy, dudx, dvdx, dudy, dvdy.  out: tex_eval<FEAT_FULL>().rgb, then for diagnosis the MIP level
// tex_lookup_width computes from the mapped width (nl - 1 + log2(max(width, 1e-8))), 1 when its zero-footprint shortcut applies,
// the mapped st.xy, 0.  (The diagnostic columns are 0 for constant and checker textures.)
PT_HD void texture_probe_row(const DScene &sc, int32_t tex, const float *in, float *out) {
    const DTexture &T = sc.texs[tex];
    const f3 v = tex_eval<FEAT_FULL>(sc, tex, mk2(in[0], in[1]), in[2], in[3], in[4], in[5]);
    for (uint32_t k = 0; k < PROBE_TEX_OUT; ++k) out[k] = 0.0f;
    out[0] = v.x; out[1] = v.y; out[2] = v.z;
    if (T.kind == 2) {
        const float width = max_nz(max_nz(fabs_(T.su * in[2]), fabs_(T.sv * in[3])), max_nz(fabs_(T.su * in[4]), fabs_(T.sv * in[5])));
        out[3] = (float)T.n_levels - 1.0f + pt_log2f(max_nz(width, 1e-8f));
        out[4] = (width <= 1e-8f && T.n_levels <= 27) ? 1.0f : 0.0f;
        out[5] = T.su * in[0] + T.du; out[6] = T.sv * in[1] + T.dv;
    }
}

// Triangle `prim` of the scene against one ray, then the hit's surface as the shade stage builds it.
// in: o.xyz, d.xyz, t_max, rx_d.xyz, ry_d.xyz (the differential rays leave from o, as the camera's do), w.xyz.
// out:  0- 4 tri_test_s: hit, t, b0, b1, b2          5- 9 tri_test_s_sel: hit, t, b0, b1, b2
//      on a hit of tri_test_s, from its b0, b1, b2 and wo = -d: tri_surface, surface_differentials, then normal_mapping for every
//      NormalMaterial wrapper around the triangle's material (make_bsdf's order):
//      10 p.xyz  13 p_error.xyz  16 n.xyz  19 ns.xyz  22 dpdu.xyz  25 dpdv.xyz  28 s_dpdu.xyz  31 s_dpdv.xyz  34 uv.xy
//      36 dudx, dvdx, dudy, dvdy  40 spawn_pair(p, p_error, n).plus.xyz  43 .minus.xyz  46 offset_ray_origin(p, p_error, n, w).xyz
//      49 number of normal_mapping steps run; the rest 0.
PT_HD void surface_probe_row(const DScene &sc, uint32_t prim, const float *in, float *out) {
    for (uint32_t k = 0; k < PROBE_SURF_OUT; ++k) out[k] = 0.0f;
    const f3 o = mk3(in[0], in[1], in[2]), d = mk3(in[3], in[4], in[5]);
    const float t_max = in[6];
    const TriRegs T = load_tri_regs(sc.shade + prim);
    const RayShear S = ray_shear(d);
    TriHit h{0.0f, 0.0f, 0.0f, 0.0f}, hs{0.0f, 0.0f, 0.0f, 0.0f};
    const bool hit = tri_test_s(o, S, t_max, T.p0, T.p1, T.p2, h);
    const bool hit_sel = tri_test_s_sel(o, S, t_max, T.p0, T.p1, T.p2, hs);
    out[0] = hit ? 1.0f : 0.0f;
    if (hit) { out[1] = h.t; out[2] = h.b0; out[3] = h.b1; out[4] = h.b2; }
    out[5] = hit_sel ? 1.0f : 0.0f;
    if (hit_sel) { out[6] = hs.t; out[7] = hs.b0; out[8] = hs.b1; out[9] = hs.b2; }
    if (!hit) return;
    Surface s = tri_surface(T, (int32_t)prim, h.b0, h.b1, h.b2, -d);
    surface_differentials(s, o, mk3(in[7], in[8], in[9]), o, mk3(in[10], in[11], in[12]));
    const DMaterial *mp = sc.mats + T.material;
    int steps = 0;
    for (; steps < 4 && mp->kind == 6; ++steps) {
        normal_mapping<FEAT_FULL>(sc, mp->tex[0], s);
        mp = sc.mats + mp->inner;
    }
    const f3 v[8] = {s.p, s.p_error, s.n, s.ns, s.dpdu, s.dpdv, s.s_dpdu, s.s_dpdv};
    for (int k = 0; k < 8; ++k) { out[10 + 3 * k] = v[k].x; out[11 + 3 * k] = v[k].y; out[12 + 3 * k] = v[k].z; }
    out[34] = s.uv.x; out[35] = s.uv.y;
    out[36] = s.dudx; out[37] = s.dvdx; out[38] = s.dudy; out[39] = s.dvdy;
    const SpawnPair sp = spawn_pair(s.p, s.p_error, s.n);
    const f3 ow = offset_ray_origin(s.p, s.p_error, s.n, mk3(in[13], in[14], in[15]));
    const f3 w[3] = {sp.plus, sp.minus, ow};
    for (int k = 0; k < 3; ++k) { out[40 + 3 * k] = w[k].x; out[41 + 3 * k] = w[k].y; out[42 + 3 * k] = w[k].z; }
    out[49] = (float)steps;
}

// The arithmetic substrate, one call per row: the transcendental stand-ins of include/ptrs_detmath.h, the binary32 helpers of
// pt_vec.h and the two cdf searches, at arguments of the test's choosing.  Every output is the raw result of the function named (an
// integer travels as the bit pattern of a float, as guide[] does); unused columns are 0.  A row is PROBE_MATH_IN floats in,
// PROBE_MATH_OUT floats out (the composites need twelve of each).
enum : uint32_t {
    MATH_SIN = 0, MATH_COS, MATH_SINCOS, MATH_TAN, MATH_LOG, MATH_LOG2, MATH_EXP, MATH_POW, MATH_ATAN2, MATH_ACOS, // pt_*f of in[0] (in[0], in[1])
    MATH_DIV,      // in[0] / in[1]
    MATH_SQRT,     // sqrt_(in[0])
    MATH_ROUND,    // floor_(in[0]), ceil_(in[0]), max0_(in[0]), clamp_(in[0], in[1], in[2])
    MATH_MINMAX,   // max_(in[0], in[1]), min_(in[0], in[1])
    MATH_MINMAX_NZ, // max_nz(in[0], in[1]), min_nz(in[0], in[1]) (domain: no +0 / -0 tie)
    MATH_U2F,      // v = bits(in[0]): (float)v * 0x1p-32f, then min_nz(PT_ONE_MINUS_EPS, .) as sobol_sample ends
    MATH_INT,      // f2i_sat(in[0]), inc_wrap(bits(in[1])), abs_mod(bits(in[2]), bits(in[3])) (0 unless the modulus is positive)
    MATH_NEXT,     // next_float_up(in[0]), next_float_down(in[0]), gamma_err(bits(in[1])), power_heuristic(in[2], in[3])
    MATH_SOLVE,    // solve_2x2(in[0..3] row-major, in[4], in[5]): solved, x0, x1
    MATH_FRAME,    // v = in[0..2]: normalize(v) 0-2, coordinate_system(v) v2 3-5, v3 6-8, spherical_theta(v) 9, spherical_phi(v) 10
    MATH_SPAWN,    // p 0-2, p_error 3-5, n 6-8, w 9-11: offset_ray_origin 0-2, spawn_pair plus 3-5, minus 6-8, spawn_from(w) 9-11
    MATH_SEARCH,   // u = in[0], size = bits(in[1]) in 2..14, cdf = in[2 .. 2 + size): find_interval_cdf, find_interval_cdf_guided
    MATH_NUM_OPS
};
PT_HD void math_probe_row(uint32_t op, const float *in, float *out) {
    for (uint32_t k = 0; k < PROBE_MATH_OUT; ++k) out[k] = 0.0f;
    const float a = in[0], b = in[1];
    switch (op) {
        case MATH_SIN: out[0] = pt_sinf(a); break;
        case MATH_COS: out[0] = pt_cosf(a); break;
        case MATH_SINCOS: pt_sincosf(a, &out[0], &out[1]); break;
        case MATH_TAN: out[0] = pt_tanf(a); break;
        case MATH_LOG: out[0] = pt_logf(a); break;
        case MATH_LOG2: out[0] = pt_log2f(a); break;
        case MATH_EXP: out[0] = pt_expf(a); break;
        case MATH_POW: out[0] = pt_powf(a, b); break;
        case MATH_ATAN2: out[0] = pt_atan2f(a, b); break;
        case MATH_ACOS: out[0] = pt_acosf(a); break;
        case MATH_DIV: out[0] = a / b; break;
        case MATH_SQRT: out[0] = sqrt_(a); break;
        case MATH_ROUND: out[0] = floor_(a); out[1] = ceil_(a); out[2] = max0_(a); out[3] = clamp_(a, b, in[2]); break;
        case MATH_MINMAX: out[0] = max_(a, b); out[1] = min_(a, b); break;
        case MATH_MINMAX_NZ: out[0] = max_nz(a, b); out[1] = min_nz(a, b); break;
        case MATH_U2F: { const uint32_t v = ptf_bits(a); out[0] = (float)v * 0x1p-32f; out[1] = min_nz(PT_ONE_MINUS_EPS, (float)v * 0x1p-32f); break; }
        case MATH_INT: {
            const int32_t m = (int32_t)ptf_bits(in[3]);
            out[0] = ptf_from_bits((uint32_t)f2i_sat(a));
            out[1] = ptf_from_bits((uint32_t)inc_wrap((int32_t)ptf_bits(b)));
            out[2] = ptf_from_bits(m > 0 ? (uint32_t)abs_mod((int32_t)ptf_bits(in[2]), m) : 0u);
            break;
        }
        case MATH_NEXT: out[0] = next_float_up(a); out[1] = next_float_down(a); out[2] = gamma_err((int32_t)ptf_bits(b)); out[3] = power_heuristic(in[2], in[3]); break;
        case MATH_SOLVE: {
            float x0 = 0.0f, x1 = 0.0f;
            const bool ok = solve_2x2(in[0], in[1], in[2], in[3], in[4], in[5], x0, x1);
            out[0] = ok ? 1.0f : 0.0f; out[1] = x0; out[2] = x1;
            break;
        }
        case MATH_FRAME: {
            const f3 v = mk3(in[0], in[1], in[2]), nv = normalize(v);
            f3 v2, v3;
            coordinate_system(v, v2, v3);
            out[0] = nv.x; out[1] = nv.y; out[2] = nv.z; out[3] = v2.x; out[4] = v2.y; out[5] = v2.z; out[6] = v3.x; out[7] = v3.y; out[8] = v3.z;
            out[9] = spherical_theta(v); out[10] = spherical_phi(v);
            break;
        }
        case MATH_SPAWN: {
            const f3 p = mk3(in[0], in[1], in[2]), pe = mk3(in[3], in[4], in[5]), n = mk3(in[6], in[7], in[8]), w = mk3(in[9], in[10], in[11]);
            const SpawnPair sp = spawn_pair(p, pe, n);
            const f3 v[4] = {offset_ray_origin(p, pe, n, w), sp.plus, sp.minus, spawn_from(sp, w)};
            for (int k = 0; k < 4; ++k) { out[3 * k] = v[k].x; out[3 * k + 1] = v[k].y; out[3 * k + 2] = v[k].z; }
            break;
        }
        case MATH_SEARCH: {
            uint32_t size = ptf_bits(b);
            size = size < 2u ? 2u : (size > 14u ? 14u : size);
            float cdf[14], guide[17];
            for (uint32_t k = 0; k < 14u; ++k) cdf[k] = k < size ? in[2u + k] : 0.0f;
            const uint32_t g = size - 1u <= 8u ? 8u : 16u; // the guide table as build_host_scene lays it out
            uint32_t cnt = 0;
            for (uint32_t k = 0; k <= g; ++k) {
                const float x = (float)k / (float)g;
                while (cnt < size && cdf[cnt] <= x) ++cnt;
                guide[k] = ptf_from_bits(cnt);
            }
            out[0] = ptf_from_bits(find_interval_cdf(cdf, size, a));
            out[1] = ptf_from_bits(find_interval_cdf_guided(cdf, size, a, guide, g));
            break;
        }
        default: break;
    }
}

// The argument checks of the texture / surface probes that need the scene (the device entry points and the host twin make the same
// ones): nullptr, or why the call is refused.  A triangle's material chain (NormalMaterial wrappers, at most 4) must stay in range.
inline const char *probe_texture_check(const HostScene &H, int32_t tex) {
    return (tex < 0 || (size_t)tex >= H.texs.size()) ? "texture index out of range" : nullptr;
}
inline const char *probe_surface_check(const HostScene &H, int32_t prim) {
    if (prim < 0 || (size_t)prim >= H.shade.size()) return "triangle index out of range";
    int32_t m = (int32_t)f2u(reinterpret_cast<const v4 *>(&H.shade[prim])[2].y);
    for (int k = 0; k <= 4; ++k) {
        if (m < 0 || (size_t)m >= H.mats.size()) return "material index out of range";
        if (H.mats[m].kind != 6 || k == 4) break;
        m = H.mats[m].inner;
    }
    return nullptr;
}

} // namespace pt
