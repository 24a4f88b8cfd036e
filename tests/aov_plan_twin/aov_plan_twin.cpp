// AOV PLAN TWIN -- TEST INFRASTRUCTURE ONLY.
// render_aov_impl itself (pathtracer-rs_amd/csrc/pt_aov.h: dense, sample ranges, tiles, band mode) on the host twin's CPU back end:
// ../host_twin/twin.cpp compiled into this library as it stands, plus a back end that adds the AOV hooks, their tile variants and
// generate_tiles as serial loops around aov_item and film_item (with P.L pointed at a plane's array).  The dilation rule is
// pt_adaptive.h's, the schedule pt_converge.h's, the ones the product calls.  Never loaded by the product.
#include "../host_twin/twin.cpp"
#include "../../pathtracer-rs_amd/csrc/pt_aov.h"
#include "../../pathtracer-rs_amd/csrc/pt_converge.h"

namespace {

struct AovBackend : HostBackend {
    // ---- the AOV hooks (HipBackend's, serially) ----
    std::vector<v4> band[4]; std::vector<f2a> band_pfilm; bool aov_band = false;
    int aov_band_begin(uint64_t n, std::string &) {
        for (auto &b : band) b.assign((size_t)n, v4{});
        band_pfilm.assign((size_t)n, f2a{});
        aov_band = true;
        return PTRS_OK;
    }
    DAov aov_arrays(bool depth_plane) {
        DAov A;
        if (aov_band) { A.albedo = band[0].data(); A.normal = band[1].data(); A.pos = band[2].data(); A.depthp = depth_plane ? band[3].data() : nullptr; A.pfilm = band_pfilm.data(); }
        else { A.albedo = P.sh_o; A.normal = P.sh_d; A.pos = P.mis_o; A.depthp = depth_plane ? P.mis_d : nullptr; A.pfilm = nullptr; }
        return A;
    }
    void aov(uint32_t planes, uint32_t off) { // k_aov: round 0's queue, entry by entry
        const DAov A = aov_arrays(true);
        for (uint32_t i = 0, n = cnt(0, Q_EXT); i < n; ++i) {
            const uint32_t pid = Q.ext[0][i];
            const f2a pf = P.pfilm[pid];
            const AovRec a = feat == FEAT_SIMPLE ? aov_item<FEAT_SIMPLE>(R, C, sc, mk2(pf.x, pf.y), P.hit[i]) : aov_item<FEAT_FULL>(R, C, sc, mk2(pf.x, pf.y), P.hit[i]);
            const uint32_t q = off + pid;
            A.albedo[q] = mkv4(a.albedo, a.coverage);
            A.normal[q] = mkv4(a.normal, a.depth);
            A.pos[q] = mkv4(a.p, u2f(a.prim));
            A.depthp[q] = mkv4(mk3(a.depth, a.coverage, 0.0f), 0.0f);
            if (A.pfilm) A.pfilm[q] = pf;
        }
    }
    // the paths of plane k's gather: p_film beside the values in band mode, the plane's array as the radiance
    DPaths plane_paths(uint32_t k) {
        const DAov A = aov_arrays(true);
        v4 *const src[AOV_PLANES] = {A.albedo, A.normal, A.depthp};
        DPaths Pk = P;
        if (A.pfilm) Pk.pfilm = A.pfilm;
        Pk.L = src[k];
        return Pk;
    }
    void film_aov(uint32_t planes, const DAovFilm &films, int32_t y0, int32_t y1, const DParams &Rf) {
        for (uint32_t k = 0; k < AOV_PLANES; ++k) {
            if (!(planes & (1u << k))) continue;
            const DPaths Pk = plane_paths(k);
            for (int32_t y = y0; y < y1; ++y) for (int32_t x = 0; x < Rf.W; ++x) film_item(Rf, S, Pk, table, films.plane[k], x, y);
        }
    }
    static void export_row(const DAov &A, uint32_t q, float *o) {
        const v4 al = A.albedo[q], nd = A.normal[q], pp = A.pos[q];
        o[0] = al.x; o[1] = al.y; o[2] = al.z; o[3] = al.w; o[4] = nd.x; o[5] = nd.y; o[6] = nd.z; o[7] = nd.w; o[8] = pp.x; o[9] = pp.y; o[10] = pp.z; o[11] = pp.w;
    }
    void export_aov(float *out, uint32_t off) {
        const DAov A = aov_arrays(true);
        for (uint32_t pid = 0; pid < R.n_paths; ++pid) {
            const PathCoord c = path_coord(R, S, pid);
            export_row(A, off + pid, out + (((size_t)c.sy * (size_t)R.NX + (size_t)c.sx) * S.spp + c.s) * AOV_SAMPLE_FLOATS);
        }
    }
    // ---- the tile variants, and TileBackend's generate_tiles (tests/adaptive_twin) ----
    void generate_tiles(const uint8_t *tile_active, int32_t tiles_x) {
        uint32_t n = 0;
        for (uint32_t pid = 0; pid < R.n_paths; ++pid) {
            const PathCoord c = path_coord(R, S, pid);
            if (!ad_pixel_active(tile_active, tiles_x, R.W, R.H, c.px, c.py)) continue;
            generate_item(R, S, C, P, pid, n); Q.ext[0][n] = pid; ++n;
        }
        cnt(0, Q_EXT) = n;
    }
    void film_aov_tiles(uint32_t planes, const DAovFilm &films, int32_t y0, int32_t y1, const DParams &Rf, const uint32_t *tile_list, uint32_t n_list, int32_t tiles_x) {
        for (uint32_t k = 0; k < AOV_PLANES; ++k) {
            if (!(planes & (1u << k))) continue;
            const DPaths Pk = plane_paths(k);
            for (uint32_t i = 0; i < n_list; ++i) {
                const int32_t tx0 = (int32_t)(tile_list[i] % (uint32_t)tiles_x) * CV_TILE, ty0 = (int32_t)(tile_list[i] / (uint32_t)tiles_x) * CV_TILE;
                for (int32_t y = std::max(ty0, y0); y < std::min(ty0 + (int32_t)CV_TILE, y1); ++y)
                    for (int32_t x = tx0; x < std::min(tx0 + (int32_t)CV_TILE, Rf.W); ++x) film_item(Rf, S, Pk, table, films.plane[k], x, y);
            }
        }
    }
    void export_aov_tiles(float *out, uint32_t off, const uint8_t *tile_active, int32_t tiles_x) {
        const DAov A = aov_arrays(true);
        for (uint32_t pid = 0; pid < R.n_paths; ++pid) {
            const PathCoord c = path_coord(R, S, pid);
            if (!ad_pixel_active(tile_active, tiles_x, R.W, R.H, c.px, c.py)) continue;
            export_row(A, off + pid, out + (((size_t)c.sy * (size_t)R.NX + (size_t)c.sx) * S.spp + c.s) * AOV_SAMPLE_FLOATS);
        }
    }
};

// range: null = every sample; tile_active: null = the dense form
int render_aov(TwinScene *s, const PtrsCamera *cam, const PtrsRenderParams *prm, const uint32_t *range, const uint8_t *tile_active, uint32_t planes, PtrsFilmPixel *const *plane_ptrs,
               float *sample_aov, PtrsStats *stats) {
    DAovFilm F;
    for (uint32_t k = 0; k < AOV_PLANES; ++k) F.plane[k] = (planes & (1u << k)) ? reinterpret_cast<v4 *>(plane_ptrs[k]) : nullptr;
    RenderJob job;
    job.sample_range = range;
    std::vector<uint8_t> flags; std::vector<uint32_t> list;
    if (tile_active) {
        ad_tile_list(tile_active, (size_t)(ad_tiles_x(prm->width) * ad_tiles_y(prm->height)), flags, list);
        if (list.empty()) { if (stats) std::memset(stats, 0, sizeof(*stats)); return PTRS_OK; }
        job.tile_active = flags.data(); job.tile_active_host = flags.data(); job.tile_list = list.data(); job.n_tile_list = (uint32_t)list.size();
    }
    AovBackend be;
    be.stack_cap = (int)std::min<uint32_t>(s->H.stack_bound, 128u);
    int rc = render_aov_impl(be, s->sc, s->H, s->H.max_depth, *cam, *prm, planes, F, sample_aov, stats, g_err, job);
    if (rc == PTRS_OK && be.overflow) { g_err = "traversal stack overflow (would corrupt LDS on the GPU)"; return PTRS_ERR_INVALID; }
    return rc;
}

bool args_ok(void *sp, const PtrsCamera *cam, const PtrsRenderParams *prm, uint32_t planes, PtrsFilmPixel *const *plane_ptrs) {
    if (!g_tables.ok) { g_err = "tables not loaded"; return false; }
    if (!sp || !cam || !prm || !plane_ptrs || planes == 0u || planes > 7u) { g_err = "null argument or bad planes"; return false; }
    for (uint32_t k = 0; k < AOV_PLANES; ++k) if ((planes & (1u << k)) && !plane_ptrs[k]) { g_err = "null plane pointer for a requested plane"; return false; }
    if (prm->width <= 0 || prm->height <= 0) { g_err = "bad render parameters"; return false; }
    return true;
}

} // namespace

extern "C" {

const char *aov_plan_twin_last_error(void) { return g_err.c_str(); }

// ptrs_render_aov (has_range = 0), ptrs_render_aov_range (tile_active null) and ptrs_render_aov_tiles on the CPU
int aov_plan_twin_render(void *sp, const PtrsCamera *cam, const PtrsRenderParams *prm, int32_t has_range, uint32_t sample_begin, uint32_t sample_end, const uint8_t *tile_active,
                         uint32_t planes, PtrsFilmPixel *const *plane_ptrs, float *sample_aov, PtrsStats *stats) {
    if (!args_ok(sp, cam, prm, planes, plane_ptrs)) return PTRS_ERR_INVALID;
    const uint32_t range[2] = {sample_begin, sample_end};
    return render_aov(static_cast<TwinScene *>(sp), cam, prm, has_range ? range : nullptr, tile_active, planes, plane_ptrs, sample_aov, stats);
}

// ptrs_render_aov_adaptive's rule, block by block (no merging of blocks: a chain of ranges gives the bits of their union)
int aov_plan_twin_render_adaptive(void *sp, const PtrsCamera *cam, const PtrsRenderParams *prm, uint32_t min_spp, const uint32_t *tile_spp, uint32_t planes, PtrsFilmPixel *const *plane_ptrs,
                                  uint64_t *samples_out) {
    if (!args_ok(sp, cam, prm, planes, plane_ptrs) || !tile_spp) { if (!tile_spp) g_err = "null argument"; return PTRS_ERR_INVALID; }
    uint32_t blocks[3 * PTRS_CONVERGE_MAX_CHECKS], n_blocks = 0;
    if (const char *m = cv_schedule(total_spp(*prm), min_spp, blocks, &n_blocks)) { g_err = m; return PTRS_ERR_INVALID; }
    const uint32_t n_tiles = (uint32_t)(ad_tiles_x(prm->width) * ad_tiles_y(prm->height));
    std::vector<uint8_t> set(n_tiles);
    uint64_t samples = 0;
    for (uint32_t k = 0; k < n_blocks; ++k) {
        for (uint32_t t = 0; t < n_tiles; ++t) set[t] = tile_spp[t] >= blocks[3 * k + 2] ? 1 : 0;
        const uint32_t range[2] = {blocks[3 * k], blocks[3 * k + 2]};
        PtrsStats st; std::memset(&st, 0, sizeof(st));
        int rc = render_aov(static_cast<TwinScene *>(sp), cam, prm, range, set.data(), planes, plane_ptrs, nullptr, &st);
        if (rc != PTRS_OK) return rc;
        samples += st.samples;
    }
    if (samples_out) *samples_out = samples;
    return PTRS_OK;
}

} // extern "C"
