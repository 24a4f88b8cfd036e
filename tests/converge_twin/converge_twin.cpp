// CONVERGE TWIN -- TEST INFRASTRUCTURE ONLY.
// (1) pt_converge.h for the CPU over whole images: cv_pixel, the tile tree and the summary in the order of k_film_error and
//     k_film_error_summary (cv_film_error_host).  (The schedule is a host function of the library itself: ptrs_converge_schedule.)
// (2) The range form of render_impl (ptrs_render_range: a sample range, a second film) on the host twin's CPU back end.  That back end
//     is ../host_twin/twin.cpp, compiled into this library as it stands -- its scenes (twin_scene_create) are the ones taken here.
// Never loaded by the product.
#include "../host_twin/twin.cpp"
#include "../../pathtracer-rs_amd/csrc/pt_converge.h"

extern "C" {

const char *converge_twin_last_error(void) { return g_err.c_str(); }

int converge_twin_film_error(int32_t W, int32_t H, const PtrsFilmPixel *film, const PtrsFilmPixel *half, PtrsTileError *tiles_out, PtrsFilmErrorSummary *summary_out) {
    if (const char *m = cv_check_args(W, H, film, half, summary_out)) { g_err = m; return PTRS_ERR_INVALID; }
    cv_film_error_host(W, H, film, half, tiles_out, summary_out);
    return PTRS_OK;
}

int converge_twin_render_range(void *sp, const PtrsCamera *cam, const PtrsRenderParams *prm, uint32_t sample_begin, uint32_t sample_end,
                               PtrsFilmPixel *film, PtrsFilmPixel *film_half, float *sample_rgb, PtrsStats *stats) {
    if (!g_tables.ok) { g_err = "tables not loaded"; return PTRS_ERR_INVALID; }
    if (!sp || !cam || !prm || !film) { g_err = "null argument"; return PTRS_ERR_INVALID; }
    TwinScene *s = static_cast<TwinScene *>(sp);
    HostBackend be;
    be.stack_cap = (int)std::min<uint32_t>(s->H.stack_bound, 128u);
    const uint32_t range[2] = {sample_begin, sample_end};
    RenderJob job;
    job.film = reinterpret_cast<v4 *>(film); job.film_half = reinterpret_cast<v4 *>(film_half); job.samples_out = sample_rgb; job.stats = stats; job.sample_range = range;
    int rc = render_impl(be, s->sc, s->H, s->H.max_depth, *cam, *prm, job, g_err);
    if (rc == PTRS_OK && be.overflow) { g_err = "traversal stack overflow (would corrupt LDS on the GPU)"; return PTRS_ERR_INVALID; }
    return rc;
}

} // extern "C"
