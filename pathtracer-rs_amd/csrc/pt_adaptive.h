// pt_adaptive.h -- adaptive sampling: which sample pixels a set of active film tiles needs, and which tiles a check freezes
// (DESIGN.md section 13).
//
// Tiles are those of the film's error (pt_converge.h): CV_TILE x CV_TILE pixels, origin (0, 0), clipped at the right and bottom
// edges, index ty * tiles_x + tx; a flag byte per tile, non-zero = active.
//   ad_pixel_active : the dilation rule.  A sample with raster pixel (px, py) lands at p in [px, px + 1) x [py, py + 1) and its
//                     footprint ceil(p - 0.5 - 2) .. floor(p - 0.5 + 2) is exactly px - 2 .. px + 2 (film.rs:66-73, radius 2): the sample
//                     pixel is active iff one pixel of that window lies in an active tile.  The window is 5 wide, a tile 16: at most
//                     two tile columns and two tile rows, four flag bytes.  k_generate_tiles, k_export_samples_tiles, the host's
//                     counts and the test twin all ask here.
//   ad_row_counts   : the active sample pixels of every sample row (what a pass traces, what the statistics count)
//   ad_freeze       : the freeze rule of ptrs_render_adaptive, a pure function of one check's tile records
//   ad_tile_list    : tile flags as a tile render takes them
//   ad_block_loop   : the loop of ptrs_render_converged and ptrs_render_adaptive over a back end's two hooks (the device's, the twin's)
// The reference renders every tile with the same sample count and has none of this.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "pt_converge.h"

namespace pt {

PT_HD bool ad_pixel_active(const uint8_t *tile_active, int32_t tiles_x, int32_t W, int32_t H, int32_t px, int32_t py) {
    const int32_t x0 = px - 2 < 0 ? 0 : px - 2, x1 = px + 2 > W - 1 ? W - 1 : px + 2;
    const int32_t y0 = py - 2 < 0 ? 0 : py - 2, y1 = py + 2 > H - 1 ? H - 1 : py + 2;
    if (x1 < x0 || y1 < y0) return false; // (never for a pixel of the sample bounds, which reach 2 beyond the film)
    const int32_t tx0 = x0 / CV_TILE, tx1 = x1 / CV_TILE, ty0 = y0 / CV_TILE, ty1 = y1 / CV_TILE;
    uint32_t a = tile_active[ty0 * tiles_x + tx0];
    if (tx1 != tx0) a |= tile_active[ty0 * tiles_x + tx1];
    if (ty1 != ty0) {
        a |= tile_active[ty1 * tiles_x + tx0];
        if (tx1 != tx0) a |= tile_active[ty1 * tiles_x + tx1];
    }
    return a != 0u;
}

inline int32_t ad_tiles_x(int32_t W) { return (W + CV_TILE - 1) / CV_TILE; }
inline int32_t ad_tiles_y(int32_t H) { return (H + CV_TILE - 1) / CV_TILE; }

// rows[sy] = the active sample pixels of sample row sy of the NX x NY sample grid whose pixel (0, 0) is raster pixel (min_x, min_y)
inline void ad_row_counts(const uint8_t *tile_active, int32_t W, int32_t H, int32_t min_x, int32_t min_y, int32_t NX, int32_t NY, std::vector<uint32_t> &rows) {
    // (ad_pixel_active summed over the row, by tile columns: the row's window touches at most two tile rows; an active tile of column tx
    // makes the raster pixels tx * 16 - 2 .. its last pixel + 2 active, and neighbouring columns' spans overlap -- each pixel counts once)
    const int32_t tiles_x = ad_tiles_x(W);
    rows.assign((size_t)NY, 0u);
    for (int32_t sy = 0; sy < NY; ++sy) {
        const int32_t py = sy + min_y, y0 = py - 2 < 0 ? 0 : py - 2, y1 = py + 2 > H - 1 ? H - 1 : py + 2;
        if (y1 < y0) continue;
        const uint8_t *r0 = tile_active + (size_t)(y0 / CV_TILE) * (size_t)tiles_x, *r1 = tile_active + (size_t)(y1 / CV_TILE) * (size_t)tiles_x;
        uint32_t n = 0;
        int32_t counted_to = min_x - 1; // the last raster pixel of the row that has been counted
        for (int32_t tx = 0; tx < tiles_x; ++tx) {
            if (!(r0[tx] | r1[tx])) continue;
            const int32_t last = tx * CV_TILE + CV_TILE - 1 < W - 1 ? tx * CV_TILE + CV_TILE - 1 : W - 1;
            const int32_t lo = std::max(tx * CV_TILE - 2, counted_to + 1), hi = std::min(last + 2, min_x + NX - 1);
            if (hi >= lo) { n += (uint32_t)(hi - lo + 1); counted_to = hi; }
        }
        rows[(size_t)sy] = n;
    }
}

// The freeze rule: a tile that took part in the block (active) and whose error is below the target is frozen -- it is never active
// again, so its pixels and with them its error stay what they are.  next[t] = 1 for the tiles that stay active, else 0 (next may be
// active itself); returns how many stay.  A tile without a valid pixel has error 0 and freezes under any target > 0; an error of
// +inf (a non-finite pixel) never does; with target = 0 nothing does (errors are never negative, never NaN).
inline uint32_t ad_freeze(const PtrsTileError *tiles, uint32_t n_tiles, float target, const uint8_t *active, uint8_t *next) {
    uint32_t n = 0;
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const uint8_t on = (active[t] != 0 && !(tiles[t].error < target)) ? 1 : 0;
        next[t] = on; n += on;
    }
    return n;
}

// What a tile render is given (RenderJob::tile_active, tile_list): the flags as 0 / 1 and the ascending list of the active tiles.
inline void ad_tile_list(const uint8_t *flags, size_t n_tiles, std::vector<uint8_t> &flags01, std::vector<uint32_t> &list) {
    flags01.resize(n_tiles); list.clear();
    for (size_t t = 0; t < n_tiles; ++t) { flags01[t] = flags[t] ? 1 : 0; if (flags[t]) list.push_back((uint32_t)t); }
}

// ---- the block loop of ptrs_render_converged and ptrs_render_adaptive (no device call: the back end is behind the hooks) -------------
// The statistics of a run of renders: counts add up, the scene's facts are the last render's, device_bytes is the largest.
inline void add_stats(PtrsStats &total, const PtrsStats &st) {
    total.samples += st.samples; total.rays_extension += st.rays_extension; total.rays_shadow += st.rays_shadow; total.rays_mis += st.rays_mis;
    total.passes += st.passes; total.kernel_launches += st.kernel_launches; total.trace_launches += st.trace_launches; total.film_launches += st.film_launches;
    total.bvh_nodes = st.bvh_nodes; total.bvh_max_depth = st.bvh_max_depth; total.device_bytes = std::max(total.device_bytes, st.device_bytes); total.lanes = st.lanes;
}

// Block by block of cv_schedule's list: the block's first half into the film and the half film, its second half into the film only,
// then the film's error, a line of the history, and the stop rule.
//   by_tile = false : every block is a dense render (no tile flags); stops when the largest tile error is below the target
//   by_tile = true  : a block runs on the tiles still active, ad_freeze takes tiles out behind every check; stops when none is left
// hooks.render(begin, end, with_half, active, st): samples [begin, end) into the film, and into the half film too when asked, on the
//   tiles flagged in `active` (n_tiles flags, 0 / 1) or densely (null); st: that render's statistics
// hooks.measure(sum, records, launches): the film's error -- the summary and, when asked (non-null), the n_tiles tile records; adds
//   what the measurement launched
// Both return PTRS_OK or the code the loop returns at once.  res.tiles_x / tiles_y are the caller's; tile_spp[t] = the samples tile t holds.
template <class Hooks>
int ad_block_loop(const uint32_t *blocks, uint32_t n_blocks, uint32_t n_tiles, float target, bool by_tile, Hooks &hooks, PtrsAdaptiveResult &res, std::vector<uint32_t> &tile_spp, PtrsStats &total) {
    std::memset(&res, 0, sizeof(res)); std::memset(&total, 0, sizeof(total));
    std::vector<uint8_t> active(n_tiles, 1);
    std::vector<PtrsTileError> records(by_tile ? n_tiles : 0u);
    tile_spp.assign(n_tiles, 0u);
    uint32_t n_active = n_tiles;
    for (uint32_t k = 0; k < n_blocks && !res.converged; ++k) {
        const uint32_t *b = blocks + 3 * k; // begin, middle, end
        for (int h = 0; h < 2; ++h) {
            PtrsStats st;
            int rc = hooks.render(b[h], b[h + 1], h == 0, by_tile ? active.data() : nullptr, st);
            if (rc != PTRS_OK) return rc;
            add_stats(total, st);
        }
        for (uint32_t t = 0; t < n_tiles; ++t) if (active[t]) tile_spp[t] = b[2];
        PtrsFilmErrorSummary sum;
        int rc = hooks.measure(sum, by_tile ? records.data() : nullptr, total.kernel_launches);
        if (rc != PTRS_OK) return rc;
        res.spp_done = b[2];
        res.history[res.n_checks].spp = b[2]; res.history[res.n_checks].tiles_active = n_active; res.history[res.n_checks].max_tile_error = sum.max_tile_error; ++res.n_checks;
        res.worst_tile = sum.worst_tile;
        if (by_tile) n_active = ad_freeze(records.data(), n_tiles, target, active.data(), active.data());
        res.converged = (by_tile ? n_active == 0u : sum.max_tile_error < target) ? 1u : 0u;
    }
    return PTRS_OK;
}

} // namespace pt
