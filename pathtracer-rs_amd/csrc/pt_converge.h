// pt_converge.h -- how far a film is from the film of half of its samples, and the schedule of a render that stops on it
// (DESIGN.md section 12).
//
// The measure is the half-buffer one of Dammertz et al.'s stopping condition: a pure function of two accumulated films, `film` with
// all samples so far and `half` with every other block of them.
//   cv_pixel    : one pixel of both films -> its error e and whether it counts
//   cv_tile_sum : the 256 slots of a 16 x 16 tile -> their sum, by the stride-halving tree (the ORDER is the contract: k_film_error
//                 runs the same tree, two steps through LDS and six across the lanes of a wave, and agrees on bits)
//   cv_tile     : sum and count -> the tile's record
//   cv_better   : the order of the summary: larger error first, then the lower tile index
// All arithmetic is binary32, one rounding per operation in the order written (-ffp-contract=off), IEEE division and square root.
// The reference renders a fixed sample count and has no such measure.
#pragma once
#include "../../include/ptrs.h"
#include "pt_scene.h"

namespace pt {

enum : int { CV_TILE = PTRS_ERROR_TILE, CV_SLOTS = CV_TILE * CV_TILE };

struct CvPixel { float e; uint32_t valid; };

PT_HD CvPixel cv_pixel(const v4 &F, const v4 &Hf) {
    CvPixel o; o.e = 0.0f; o.valid = 0u;
    if (!(F.w > 0.0f && Hf.w > 0.0f)) return o; // an empty pixel of either film: e = 0, not counted
    const float ir = F.x / F.w, ig = F.y / F.w, ib = F.z / F.w;
    const float ar = Hf.x / Hf.w, ag = Hf.y / Hf.w, ab = Hf.z / Hf.w;
    const float d = (fabs_(ir - ar) + fabs_(ig - ag)) + fabs_(ib - ab);
    const float s = (ir + ig) + ib;
    float e = d / sqrt_(max_(s, 1.0e-3f));
    if (!(e < PT_INF)) e = PT_INF; // NaN or infinite: such a film never converges, it is never silently fine (e is never negative)
    o.e = e; o.valid = 1u;
    return o;
}

// v[i] += v[i + off] for i < off, off = 128, 64, ..., 1; the sum ends up in v[0] (v is overwritten)
inline float cv_tile_sum(float *v /* CV_SLOTS */) {
    for (int off = CV_SLOTS / 2; off > 0; off >>= 1)
        for (int i = 0; i < off; ++i) v[i] = v[i] + v[i + off];
    return v[0];
}

PT_HD PtrsTileError cv_tile(float sum, uint32_t valid) {
    PtrsTileError t; t.valid = valid;
    t.error = valid ? sum / (float)valid : 0.0f;
    return t;
}

// tile (ea, ia) comes before tile (eb, ib) in the summary (tile errors are never NaN and never negative)
PT_HD bool cv_better(float ea, uint32_t ia, float eb, uint32_t ib) { return ea > eb || (ea == eb && ia < ib); }

// ---- host side: argument checks and the schedule (no device call) ------------------------------------------------------------
inline const char *cv_check_args(int32_t W, int32_t H, const void *film, const void *half, const void *summary) {
    if (!film || !half || !summary) return "null argument";
    if (W <= 0 || H <= 0) return "film width and height must be positive";
    if (film == half) return "film and half must be two films";
    if ((uint64_t)W * (uint64_t)H >= (1ull << 31)) return "film too large for the error measure";
    return nullptr;
}

// The blocks of a render that doubles its samples until it has converged: block 0 = [0, min_spp), block k = [n, 2n).  Three numbers per
// block: begin, middle, end -- [begin, middle) goes to the film and the half film, [middle, end) to the film only.
inline const char *cv_schedule(uint32_t spp, uint32_t min_spp, uint32_t *blocks /* 3 x PTRS_CONVERGE_MAX_CHECKS */, uint32_t *n_blocks) {
    if (!blocks || !n_blocks) return "null argument";
    if (spp == 0u || (spp & (spp - 1u)) != 0u) return "render_converged: the ceiling spp must be a power of two";
    if (min_spp < 2u || (min_spp & (min_spp - 1u)) != 0u || min_spp > spp) return "render_converged: min_spp must be a power of two in 2 .. spp";
    uint32_t k = 0, n = 0;
    while (n < spp) {
        const uint32_t b = n, e = n ? 2u * n : min_spp;
        blocks[3 * k] = b; blocks[3 * k + 1] = b + (e - b) / 2u; blocks[3 * k + 2] = e;
        ++k; n = e;
    }
    *n_blocks = k; // at most log2(spp / min_spp) + 1 <= 31
    return nullptr;
}

// host twin of k_film_error + k_film_error_summary over whole images (tests/converge_twin; the product runs the kernels)
inline void cv_film_error_host(int32_t W, int32_t H, const PtrsFilmPixel *film, const PtrsFilmPixel *half, PtrsTileError *tiles /* may be null */, PtrsFilmErrorSummary *sum) {
    const int32_t tx_n = (W + CV_TILE - 1) / CV_TILE, ty_n = (H + CV_TILE - 1) / CV_TILE;
    PtrsFilmErrorSummary s; s.max_tile_error = 0.0f; s.worst_tile = 0u; s.valid_pixels = 0u; s.tiles_x = (uint32_t)tx_n; s.tiles_y = (uint32_t)ty_n;
    bool first = true;
    for (int32_t ty = 0; ty < ty_n; ++ty)
        for (int32_t tx = 0; tx < tx_n; ++tx) {
            float v[CV_SLOTS]; uint32_t valid = 0u;
            for (int32_t ly = 0; ly < CV_TILE; ++ly)
                for (int32_t lx = 0; lx < CV_TILE; ++lx) {
                    const int32_t x = tx * CV_TILE + lx, y = ty * CV_TILE + ly;
                    float e = 0.0f;
                    if (x < W && y < H) {
                        const PtrsFilmPixel &f = film[(size_t)y * (size_t)W + (size_t)x], &h = half[(size_t)y * (size_t)W + (size_t)x];
                        v4 a, b; a.x = f.rgb[0]; a.y = f.rgb[1]; a.z = f.rgb[2]; a.w = f.weight; b.x = h.rgb[0]; b.y = h.rgb[1]; b.z = h.rgb[2]; b.w = h.weight;
                        const CvPixel p = cv_pixel(a, b);
                        e = p.e; valid += p.valid;
                    }
                    v[ly * CV_TILE + lx] = e;
                }
            const PtrsTileError t = cv_tile(cv_tile_sum(v), valid);
            const uint32_t ti = (uint32_t)(ty * tx_n + tx);
            if (tiles) tiles[ti] = t;
            if (first || cv_better(t.error, ti, s.max_tile_error, s.worst_tile)) { s.max_tile_error = t.error; s.worst_tile = ti; first = false; }
            s.valid_pixels += t.valid;
        }
    *sum = s;
}

} // namespace pt
