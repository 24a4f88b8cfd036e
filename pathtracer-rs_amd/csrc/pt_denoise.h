// pt_denoise.h -- edge-avoiding a-trous filter of a low-spp film, guided by the first-hit planes of pt_aov.h.
//
// A pure function of four accumulated films (beauty, albedo, normal, depth + coverage).  Per pixel:
//   dn_prepare  : the films' sums -> colour over albedo, coverage | unit normal, depth | the albedo it was divided by
//   dn_atrous   : one iteration at one pixel: 25 taps `step` pixels apart, weighted by the B3 spline and exp(-e), e from the colour,
//                 normal + coverage and relative-depth distances to the tap; the taps come from a functor, so the kernel that reads them
//                 from global memory, the one that reads them from an LDS tile and the host twin run the same arithmetic
//   dn_finish   : times the albedo, weight 1
// All arithmetic is binary32, one rounding per operation in the order written (-ffp-contract=off); pt_expf is binary64 rounded once.
// The reference has no such filter.
#pragma once
#include "../../include/ptrs.h"
#include "pt_scene.h"

namespace pt {

// What the iterations read per pixel: x = (colour.rgb, coverage), an empty pixel (no weight: never a tap, zeros in the output)
// carries a NaN as its coverage; g = (unit normal.xyz, depth); a = the albedo the colour was divided by.
struct DnPixel { v4 x, g, a; };
struct DnIter { // one iteration's constants
    int32_t W, H, step;
    float sc2, sn2, sd2; // the squared sigmas; a term whose sigma is <= 0 is dropped (use bit 0 colour, 1 normal, 2 depth)
    uint32_t use;
};

PT_HD bool dn_ok(const v4 &x) { return x.w == x.w; }
PT_HD float dn_empty_mark() { return ptf_from_bits(0x7fc00000u); }

PT_HD DnPixel dn_prepare(v4 B, v4 A, v4 N, v4 D, bool demodulate) {
    DnPixel o;
    const float w = B.w;
    if (!(w > 0.0f)) {
        o.x = mkv4(splat3(0.0f), dn_empty_mark()); o.g = mkv4(splat3(0.0f), 0.0f); o.a = mkv4(splat3(1.0f), 0.0f);
        return o;
    }
    const f3 c = mk3(B.x / w, B.y / w, B.z / w);
    const float cov = D.y / w;
    const float z = D.y > 0.0f ? D.x / D.y : 0.0f;
    f3 n = mk3(N.x / w, N.y / w, N.z / w);
    const float l = sqrt_((n.x * n.x + n.y * n.y) + n.z * n.z);
    n = l > 0.0f ? mk3(n.x / l, n.y / l, n.z / l) : splat3(0.0f);
    f3 a = splat3(1.0f);
    if (demodulate) { // the uncovered share of the pixel counts as albedo 1
        const float t = w - D.y;
        const float ax = (A.x + t) / w, ay = (A.y + t) / w, az = (A.z + t) / w;
        a = mk3(ax > 0.01f ? ax : 0.01f, ay > 0.01f ? ay : 0.01f, az > 0.01f ? az : 0.01f);
    }
    o.x = mkv4(mk3(c.x / a.x, c.y / a.y, c.z / a.z), cov);
    o.g = mkv4(n, z);
    o.a = mkv4(a, 0.0f);
    return o;
}

// One iteration at a pixel with colour xp and guide gp.  fetch(dx, dy, xq, gq): the tap at p + step * (dx, dy); false when it lies
// outside the image or is empty.  dy is the outer loop, dx the inner one, both from -2 to 2; the sums are formed in that order.
template <class Fetch>
PT_HD v4 dn_atrous(const DnIter &it, v4 xp, v4 gp, Fetch &&fetch) {
    if (!dn_ok(xp)) return xp;
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            v4 xq, gq;
            if (!fetch(dx, dy, xq, gq)) continue;
            float e = 0.0f;
            if (it.use & 1u) {
                const float dr = xp.x - xq.x, dg = xp.y - xq.y, db = xp.z - xq.z;
                e = e + ((dr * dr + dg * dg) + db * db) / it.sc2;
            }
            if (it.use & 2u) {
                const float d0 = gp.x - gq.x, d1 = gp.y - gq.y, d2 = gp.z - gq.z, dc = xp.w - xq.w;
                e = e + (((d0 * d0 + d1 * d1) + d2 * d2) + dc * dc) / it.sn2;
            }
            if (it.use & 4u) {
                const float m0 = gp.w > gq.w ? gp.w : gq.w;
                const float m = m0 > 1e-30f ? m0 : 1e-30f;
                const float r = (gp.w - gq.w) / m;
                e = e + (r * r) / it.sd2;
            }
            const float wt = (h[dy + 2] * h[dx + 2]) * pt_expf(-e);
            nr = nr + wt * xq.x; ng = ng + wt * xq.y; nb = nb + wt * xq.z;
            den = den + wt;
        }
    return mkv4(mk3(nr / den, ng / den, nb / den), xp.w); // the centre tap has wt = 9 / 64: den > 0
}

PT_HD v4 dn_finish(v4 x, v4 a) {
    if (!dn_ok(x)) return mkv4(splat3(0.0f), 0.0f);
    return mkv4(mk3(x.x * a.x, x.y * a.y, x.z * a.z), 1.0f);
}

// The checks of ptrs_denoise that need no device; null: fine
inline const char *dn_check_params(const PtrsDenoiseParams &p) {
    if (p.iterations < 1 || p.iterations > PTRS_DENOISE_MAX_ITERATIONS) return "iterations must be 1 .. 8";
    const float s[3] = {p.sigma_color, p.sigma_normal, p.sigma_depth};
    for (float v : s) if (!(v == v) || isinf_(v)) return "a sigma is not finite";
    return nullptr;
}
// Iteration i's constants: step 2^i, colour sigma sigma_color * 2^-i (exact), every sigma squared with one rounding
inline DnIter dn_iter(const PtrsDenoiseParams &p, int32_t W, int32_t H, int i) {
    DnIter it;
    it.W = W; it.H = H; it.step = 1 << i;
    const float sc = p.sigma_color * ptf_from_bits((uint32_t)(127 - i) << 23);
    it.sc2 = sc * sc; it.sn2 = p.sigma_normal * p.sigma_normal; it.sd2 = p.sigma_depth * p.sigma_depth;
    it.use = (p.sigma_color > 0.0f ? 1u : 0u) | (p.sigma_normal > 0.0f ? 2u : 0u) | (p.sigma_depth > 0.0f ? 4u : 0u);
    return it;
}

} // namespace pt
