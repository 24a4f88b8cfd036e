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
// The reference renders every tile with the same sample count and has none of this.
#pragma once
#include <algorithm>
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

} // namespace pt
