// ADAPTIVE TWIN -- TEST INFRASTRUCTURE ONLY.
// The tile form of render_impl (ptrs_render_tiles) and the adaptive loop (ptrs_render_adaptive) on the host twin's CPU back end:
// ../host_twin/twin.cpp compiled into this library as it stands, plus a back end that adds the three tile hooks and runs the shared
// stage functions serially.  The freeze rule and the dilation rule are pt_adaptive.h's, the ones the product calls; the film's error is
// pt_converge.h's host form.  Never loaded by the product.
#include "../host_twin/twin.cpp"
#include "../../pathtracer-rs_amd/csrc/pt_adaptive.h"
#include "../../pathtracer-rs_amd/csrc/pt_converge.h"

namespace {

struct TileBackend : HostBackend {
    void generate_tiles(const uint8_t *tile_active, int32_t tiles_x) {
        uint32_t n = 0;
        for (uint32_t pid = 0; pid < R.n_paths; ++pid) {
            const PathCoord c = path_coord(R, S, pid);
            if (!ad_pixel_active(tile_active, tiles_x, R.W, R.H, c.px, c.py)) continue;
            generate_item(R, S, C, P, pid, n); Q.ext[0][n] = pid; ++n;
        }
        cnt(0, Q_EXT) = n;
    }
    void film_tiles(v4 *film_px, int32_t y0, int32_t y1, const uint32_t *tile_list, uint32_t n_list, int32_t tiles_x) {
        for (uint32_t i = 0; i < n_list; ++i) {
            const int32_t tx0 = (int32_t)(tile_list[i] % (uint32_t)tiles_x) * CV_TILE, ty0 = (int32_t)(tile_list[i] / (uint32_t)tiles_x) * CV_TILE;
            for (int32_t y = std::max(ty0, y0); y < std::min(ty0 + (int32_t)CV_TILE, y1); ++y)
                for (int32_t x = tx0; x < std::min(tx0 + (int32_t)CV_TILE, R.W); ++x) film_item(R, S, P, table, film_px, x, y);
        }
    }
    void export_samples_tiles(float *out, const uint8_t *tile_active, int32_t tiles_x) {
        for (uint32_t pid = 0; pid < R.n_paths; ++pid) {
            const PathCoord c = path_coord(R, S, pid);
            if (!ad_pixel_active(tile_active, tiles_x, R.W, R.H, c.px, c.py)) continue;
            const size_t o = (((size_t)c.sy * (size_t)R.NX + (size_t)c.sx) * S.spp + c.s) * 3;
            out[o] = P.L[pid].x; out[o + 1] = P.L[pid].y; out[o + 2] = P.L[pid].z;
        }
    }
};

int render_tiles(TwinScene *s, const PtrsCamera *cam, const PtrsRenderParams *prm, uint32_t sample_begin, uint32_t sample_end, const uint8_t *tile_active,
                 PtrsFilmPixel *film, PtrsFilmPixel *film_half, float *sample_rgb, PtrsStats *stats) {
    const uint32_t n_tiles = (uint32_t)(ad_tiles_x(prm->width) * ad_tiles_y(prm->height));
    std::vector<uint8_t> flags; std::vector<uint32_t> list;
    ad_tile_list(tile_active, n_tiles, flags, list);
    if (list.empty()) { if (stats) std::memset(stats, 0, sizeof(*stats)); return PTRS_OK; }
    TileBackend be;
    be.stack_cap = (int)std::min<uint32_t>(s->H.stack_bound, 128u);
    const uint32_t range[2] = {sample_begin, sample_end};
    RenderJob job;
    job.film = reinterpret_cast<v4 *>(film); job.film_half = reinterpret_cast<v4 *>(film_half); job.samples_out = sample_rgb; job.stats = stats; job.sample_range = range;
    job.tile_active = flags.data(); job.tile_active_host = flags.data(); job.tile_list = list.data(); job.n_tile_list = (uint32_t)list.size();
    int rc = render_impl(be, s->sc, s->H, s->H.max_depth, *cam, *prm, job, g_err);
    if (rc == PTRS_OK && be.overflow) { g_err = "traversal stack overflow (would corrupt LDS on the GPU)"; return PTRS_ERR_INVALID; }
    return rc;
}

} // namespace

extern "C" {

const char *adaptive_twin_last_error(void) { return g_err.c_str(); }

uint32_t adaptive_twin_freeze(const PtrsTileError *tiles, uint32_t n_tiles, float target, const uint8_t *active, uint8_t *next) { return ad_freeze(tiles, n_tiles, target, active, next); }

int adaptive_twin_film_error(int32_t W, int32_t H, const PtrsFilmPixel *film, const PtrsFilmPixel *half, PtrsTileError *tiles_out, PtrsFilmErrorSummary *summary_out) {
    if (const char *m = cv_check_args(W, H, film, half, summary_out)) { g_err = m; return PTRS_ERR_INVALID; }
    cv_film_error_host(W, H, film, half, tiles_out, summary_out);
    return PTRS_OK;
}

int adaptive_twin_render_tiles(void *sp, const PtrsCamera *cam, const PtrsRenderParams *prm, uint32_t sample_begin, uint32_t sample_end, const uint8_t *tile_active,
                               PtrsFilmPixel *film, PtrsFilmPixel *film_half, float *sample_rgb, PtrsStats *stats) {
    if (!g_tables.ok) { g_err = "tables not loaded"; return PTRS_ERR_INVALID; }
    if (!sp || !cam || !prm || !film || !tile_active) { g_err = "null argument"; return PTRS_ERR_INVALID; }
    if (prm->width <= 0 || prm->height <= 0) { g_err = "bad render parameters"; return PTRS_ERR_INVALID; }
    return render_tiles(static_cast<TwinScene *>(sp), cam, prm, sample_begin, sample_end, tile_active, film, film_half, sample_rgb, stats);
}

// ptrs_render_adaptive's loop (ad_block_loop, the one the product runs) over the twin's tile form and the host form of the film's error.
// history3: per check {spp, tiles that took part} as two uint32 and the largest tile error's bits as the third; tile_errors (may be
// null): the tile records of every check, n_checks x n_tiles.
int adaptive_twin_render_adaptive(void *sp, const PtrsCamera *cam, const PtrsRenderParams *prm, float target, uint32_t min_spp, PtrsFilmPixel *film, PtrsFilmPixel *half,
                                  uint32_t *tile_spp, uint32_t *history3, uint32_t *n_checks_out, uint32_t *converged_out, PtrsTileError *tile_errors, uint64_t *samples_out) {
    if (!g_tables.ok) { g_err = "tables not loaded"; return PTRS_ERR_INVALID; }
    if (!sp || !cam || !prm || !film || !half || !tile_spp || !history3 || !n_checks_out || !converged_out) { g_err = "null argument"; return PTRS_ERR_INVALID; }
    uint32_t blocks[3 * PTRS_CONVERGE_MAX_CHECKS], n_blocks = 0;
    if (const char *m = cv_schedule(total_spp(*prm), min_spp, blocks, &n_blocks)) { g_err = m; return PTRS_ERR_INVALID; }
    const uint32_t n_tiles = (uint32_t)(ad_tiles_x(prm->width) * ad_tiles_y(prm->height));
    struct Hooks {
        TwinScene *s; const PtrsCamera *cam; const PtrsRenderParams *prm; PtrsFilmPixel *film, *half; PtrsTileError *tile_errors; uint32_t n_tiles;
        int render(uint32_t begin, uint32_t end, bool with_half, const uint8_t *active, PtrsStats &st) { return render_tiles(s, cam, prm, begin, end, active, film, with_half ? half : nullptr, nullptr, &st); }
        int measure(PtrsFilmErrorSummary &sum, PtrsTileError *records, uint64_t &) {
            cv_film_error_host(prm->width, prm->height, film, half, records, &sum);
            if (tile_errors) { std::memcpy(tile_errors, records, (size_t)n_tiles * sizeof(PtrsTileError)); tile_errors += n_tiles; }
            return PTRS_OK;
        }
    } hooks{static_cast<TwinScene *>(sp), cam, prm, film, half, tile_errors, n_tiles};
    PtrsAdaptiveResult res; PtrsStats total; std::vector<uint32_t> spp_of;
    int rc = ad_block_loop(blocks, n_blocks, n_tiles, target, true, hooks, res, spp_of, total);
    if (rc != PTRS_OK) return rc;
    std::memcpy(tile_spp, spp_of.data(), (size_t)n_tiles * 4);
    for (uint32_t i = 0; i < res.n_checks; ++i) { history3[3 * i] = res.history[i].spp; history3[3 * i + 1] = res.history[i].tiles_active; std::memcpy(&history3[3 * i + 2], &res.history[i].max_tile_error, 4); }
    *n_checks_out = res.n_checks; *converged_out = res.converged;
    if (samples_out) *samples_out = total.samples;
    return PTRS_OK;
}

} // extern "C"
