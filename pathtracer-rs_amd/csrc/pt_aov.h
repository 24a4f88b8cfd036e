// pt_aov.h -- first-hit feature planes (albedo, shading normal, depth + coverage) on the camera samples.
//
// A denoiser or a compositor wants, next to the radiance film, what the camera rays saw: filtered onto the film by exactly the samples
// and weights of the beauty image.  Everything that is needed sits in the pipeline after round 0 -- the hit (triangle id, barycentrics)
// in P.hit, the film position in P.pfilm -- so an AOV call is a render cut after its first extension: generate, extend(0), then
//   aov_item          : camera_ray -> tri_surface -> surface_differentials -> the NormalMaterial chain (make_bsdf's order) -> the values
//   render_aov_impl   : render_impl's set-up, pass plan and lanes around those three stages and the plane films; a sample range and a
//                       set of film tiles restrict it like render_impl
// Specular first hits are not followed: a mirror shows the mirror's own surface.  The reference has no such call.
#pragma once
#include "pt_render.h"

namespace pt {

enum : uint32_t { AOV_ALBEDO = 0, AOV_NORMAL = 1, AOV_DEPTH = 2, AOV_PLANES = 3, AOV_SAMPLE_FLOATS = 12 };

// What k_aov leaves per path slot, in path-state arrays an AOV pass has no other use for (max_depth 0: no vertex is shaded, nothing
// is connected).  depthp (the depth plane as the film gathers it: depth, coverage, 0) is written only for the per-plane film launches.
struct DAov {
    v4 *albedo; // [pid]: albedo.rgb, coverage
    v4 *normal; // [pid]: shading normal (world space), depth
    v4 *pos;    // [pid]: hit position, the triangle id's bits
    v4 *depthp; // [pid] or null: depth, coverage, 0, 0
    f2a *pfilm; // [pid] or null: a copy of p_film beside the values (band mode of render_aov_impl: the arrays outlive the pass)
};
struct DAovFilm { v4 *plane[AOV_PLANES]; }; // film of plane k (device memory, W x H), null when the plane is not asked for

struct AovRec { f3 albedo; float coverage; f3 normal; float depth; f3 p; uint32_t prim; };

// The texture slot that holds a material kind's base colour; -1: the kind has none (Mirror reflects everything: 1, 1, 1).
PT_HD int aov_albedo_slot(int32_t kind) {
    switch (kind) {
        case PTRS_MAT_MATTE: case PTRS_MAT_GLASS: case PTRS_MAT_DISNEY: case PTRS_MAT_SUBSTRATE: return 0; // kd, kr, color, kd
        case PTRS_MAT_METAL: return 2;                                                                    // r
        default: return -1;
    }
}

// The planes' values of one camera sample: p_film and the hit word of round 0 (P.hit: packed triangle id, barycentrics).
// `ray`: under a thin lens (C.lens_radius > 0) the ray generate_item made, origin and direction (its bits, read back from round 0's queue);
// without a lens it is not read, the pinhole ray is a function of p_film.
template <int FEAT>
PT_HD AovRec aov_item(const DParams &R, const DCamera &C, const DScene &sc, f2 pf, u4 hit, const f3 *ray = nullptr) {
    AovRec a;
    a.albedo = a.normal = a.p = splat3(0.0f); a.coverage = 0.0f; a.depth = 0.0f; a.prim = 0xffffffffu;
    const int32_t prim = hit_prim(hit.x);
    if (prim < 0) return a;
    const CamRay cr = (ray && C.lens_radius > 0.0f) ? first_vertex_ray(C, pf, R.inv_sqrt_spp, ray[0], ray[1]) : camera_ray(C, pf, R.inv_sqrt_spp);
    const TriRegs T = load_tri_regs(sc.shade + prim);
    Surface s = tri_surface(T, prim, u2f(hit.y), u2f(hit.z), u2f(hit.w), -cr.d);
    surface_differentials(s, cr.o, cr.rx_d, cr.o, cr.ry_d);
    const DMaterial *mp = sc.mats + T.material;
    if (FEAT & FEAT_NORMAL) {
        for (int guard = 0; guard < 4 && mp->kind == PTRS_MAT_NORMAL; ++guard) {
            normal_mapping<FEAT>(sc, mp->tex[0], s);
            mp = sc.mats + mp->inner;
        }
    }
    const DMaterial &m = *mp;
    const int slot = aov_albedo_slot(m.kind);
    a.albedo = (slot >= 0 && m.tex[slot] >= 0) ? mat_tex<FEAT>(sc, m, slot, s) : splat3(1.0f);
    a.coverage = 1.0f;
    a.normal = s.ns;
    a.p = s.p;
    a.depth = len(s.p - cr.o);
    a.prim = (uint32_t)prim;
    return a;
}

// One sample's 12 floats of ptrs_render_aov's sample_aov: albedo, coverage, normal, depth, position, triangle id bits
PT_HD void aov_sample_row(const AovRec &a, float *o) {
    o[0] = a.albedo.x; o[1] = a.albedo.y; o[2] = a.albedo.z; o[3] = a.coverage;
    o[4] = a.normal.x; o[5] = a.normal.y; o[6] = a.normal.z; o[7] = a.depth;
    o[8] = a.p.x; o[9] = a.p.y; o[10] = a.p.z; o[11] = u2f(a.prim);
}

// The AOV call: render_impl's set-up and pass plan (render_setup, plan_passes: a plane's weight channel is then formed by the very
// additions of the beauty film's) with max_depth forced to 0, and per pass
//     pass_begin -> generate -> extend(0) -> aov -> the plane films, chained in pass order.
// The survival profile of the scene (be.learn / be.tail_round) belongs to beauty renders and is neither read nor fed.
// A plan that cuts the band's ROWS into blocks (a band of one sample exceeds the pass capacity: then every pass holds one sample index)
// would hand a pixel at a block boundary its samples block by block, where a plan of whole-band passes hands them over sample by
// sample: other float32 sums.  The planes must not depend on the pass size, so such a plan runs in BAND MODE: the same passes, ordered
// sample index first, leave their values (and p_film) in arrays of the whole band (72 bytes per sample pixel), and when a sample
// index's last block is through ONE film gather runs over the band -- the order of a whole-band pass: sample, x, y.  On one lane: the
// stream orders the blocks, the gather and the next sample's blocks.
//
// Sample ranges and tiles.  `job` carries RenderJob's sample_range and tile fields, nothing else of it is read.
// A range runs the passes over [begin, end) and leaves sampler, sample layout and differentials those of the whole render: in either
// mode a pixel receives its samples sample index by sample index, so ranges that tile [0, spp) in order form the dense call's sums.
// The tile form keeps the dense pass's slots and plan (render_impl's tile form): generate_tiles makes paths for the active sample
// pixels only, k_aov walks that queue, the gather runs one workgroup per active tile and reads only slots of active sample pixels --
// the others hold what earlier passes (or, in band mode, earlier sample indices and calls) left there.  A pass whose rows hold no active
// sample pixel is skipped; in band mode the gather follows the last block of the sample index that was not.
template <class BE, class = void> struct has_aov_tile_hooks : std::false_type {};
template <class BE> struct has_aov_tile_hooks<BE, std::void_t<decltype(std::declval<BE &>().export_aov_tiles((float *)nullptr, 0u, (const uint8_t *)nullptr, (int32_t)0))>> : has_tile_hooks<BE> {};

template <class BE>
int render_aov_impl(BE &be, const DScene &sc, const HostScene &sc_host_feat, uint32_t bvh_depth, const PtrsCamera &cam, const PtrsRenderParams &prm_in,
                    uint32_t planes, const DAovFilm &films /* backend memory, W*H each */, float *samples_out /* backend memory or null */, PtrsStats *stats, std::string &err,
                    const RenderJob &job_in = RenderJob{}) {
    using clock = std::chrono::steady_clock;
    auto t_begin = clock::now();
    if (prm_in.max_depth < 0) { err = "bad render parameters"; return PTRS_ERR_INVALID; }
    PtrsRenderParams prm = prm_in;
    prm.max_depth = 0; // the pass ends behind its first extension: the epilogue buckets nothing
    RenderJob job; // (what an AOV call can be asked for)
    job.sample_range = job_in.sample_range; job.tile_active = job_in.tile_active; job.tile_active_host = job_in.tile_active_host; job.tile_list = job_in.tile_list; job.n_tile_list = job_in.n_tile_list;
    RenderSetup u;
    int rc = render_setup(be, bvh_depth, cam, prm, job, u, err);
    if (rc != PTRS_OK) return rc;
    const SampleGrid &g = u.g;
    const uint32_t sb = u.sb, se = u.se, ns = se - sb;
    const int32_t rb = u.rb, re = u.re, srow0 = u.srow0, srow1 = u.srow1;
    DParams R = u.R;

    const uint64_t band_rows = (uint64_t)(srow1 - srow0);
    constexpr bool tile_hooks = has_aov_tile_hooks<BE>::value;
    const bool tiled = job.tile_active != nullptr;
    if (tiled && !tile_hooks) { err = "this back end has no tile form"; return PTRS_ERR_UNSUPPORTED; }
    const int32_t tiles_x = ad_tiles_x(prm.width);
    std::vector<uint32_t> row_active;
    uint64_t job_pixels = band_rows * (uint64_t)g.NX;
    if (tiled) { // (render_impl's tile form: what is traced and counted are the active sample pixels of the rows)
        ad_row_counts(job.tile_active_host, prm.width, prm.height, g.min_x, g.min_y, g.NX, g.NY, row_active);
        job_pixels = 0;
        for (int32_t r = srow0; r < srow1; ++r) job_pixels += row_active[(size_t)r];
        if (job_pixels == 0) { // no tile is active: no device call
            if (stats) std::memset(stats, 0, sizeof(*stats));
            return PTRS_OK;
        }
    }
    const uint32_t n_lanes = std::max(1u, be.lanes(job_pixels * (uint64_t)ns, sc_host_feat.kinds_present, false, ns));
    uint64_t capacity = std::min<uint64_t>(1ull << 27, prm.paths_per_pass ? prm.paths_per_pass : be.auto_capacity(n_lanes, sc_host_feat.kinds_present));
    if (capacity < (uint64_t)g.NX) capacity = (uint64_t)g.NX;
    PassPlan pp;
    if (!plan_passes(band_rows, (uint64_t)g.NX, ns, capacity, n_lanes, prm.paths_per_pass != 0, pp)) { err = "pass too large"; return PTRS_ERR_INVALID; }
    const uint64_t rows_per_pass = pp.rows_per_pass, samples_per_pass = pp.samples_per_pass;

    const uint32_t count_rows = 2u; // round 0, and the row its kernels may look ahead to
    const int feat = scene_features(sc_host_feat), feat_trace = scene_trace_features(sc_host_feat);
    rc = be.begin(sc, u.S, u.C, (uint32_t)pp.max_paths, count_rows, bvh_depth, prm.flags, feat, feat_trace, err);
    if (rc != PTRS_OK) return rc;

    PtrsStats st;
    std::memset(&st, 0, sizeof(st));
    std::vector<uint32_t> counts((size_t)count_rows * Q_STRIDE);
    const bool band_mode = rows_per_pass < band_rows; // (samples_per_pass == 1)
    if (band_mode) {
        if (band_rows * (uint64_t)g.NX > (1ull << 27)) { err = "band too large for the pass capacity"; return PTRS_ERR_UNSUPPORTED; }
        if ((rc = be.aov_band_begin(band_rows * (uint64_t)g.NX, err)) != PTRS_OK) return rc;
    }
    struct Pass { int32_t r0, r1; uint32_t s0, s1; bool last_block; uint64_t pixels /* the sample pixels it traces */; };
    std::vector<Pass> plan;
    auto add_pass = [&](int32_t r0, uint32_t s0, uint32_t s1) {
        const int32_t r1 = std::min<int32_t>(srow1, r0 + (int32_t)rows_per_pass);
        uint64_t pixels = (uint64_t)(r1 - r0) * (uint64_t)g.NX;
        if (tiled) { pixels = 0; for (int32_t r = r0; r < r1; ++r) pixels += row_active[(size_t)r]; }
        if (pixels == 0) return; // (tile form: a pass whose sample rows hold no active sample pixel is skipped and not counted)
        plan.push_back(Pass{r0, r1, s0, s1, true, pixels});
    };
    if (band_mode) {
        for (uint32_t s0 = sb; s0 < se; ++s0) {
            for (int32_t r0 = srow0; r0 < srow1; r0 += (int32_t)rows_per_pass) add_pass(r0, s0, s0 + 1u);
            for (size_t i = plan.size(); i-- > 0 && plan[i].s0 == s0;) plan[i].last_block = i + 1 == plan.size(); // the gather follows the sample index's last block
        }
    } else {
        for (int32_t r0 = srow0; r0 < srow1; r0 += (int32_t)rows_per_pass)
            for (uint32_t s0 = sb; s0 < se; s0 += (uint32_t)samples_per_pass) add_pass(r0, s0, (uint32_t)std::min<uint64_t>(se, (uint64_t)s0 + samples_per_pass));
    }
    struct Pending { bool active = false; uint32_t n_paths = 0; };
    std::vector<Pending> pending(n_lanes);
    auto finish = [&](uint32_t lane) { // the counters of the pass a lane ran last (waits for that lane only)
        Pending &pd = pending[lane];
        if (!pd.active) return;
        be.select(lane);
        be.read_counts(counts.data(), 1u);
        st.rays_extension += counts[Q_EXT];
        st.rays_shadow += counts[Q_SHADOW];
        st.rays_mis += counts[Q_MIS];
        st.samples += pd.n_paths;
        st.passes += 1;
        pd.active = false;
    };
    uint32_t pass_no = 0;
    for (const Pass &ps : plan) {
        const uint32_t lane = band_mode ? 0u : pass_no % n_lanes;
        finish(lane);
        be.select(lane);
        R.row0 = ps.r0; R.row1 = ps.r1; R.s0 = ps.s0; R.s1 = ps.s1;
        R.n_paths = (uint32_t)(ps.r1 - ps.r0) * (uint32_t)g.NX * (ps.s1 - ps.s0);
        const uint32_t off = band_mode ? (uint32_t)(ps.r0 - srow0) * (uint32_t)g.NX : 0u; // the pass's first slot in the band's arrays
        const uint32_t n_traced = tiled ? (uint32_t)(ps.pixels * (uint64_t)(ps.s1 - ps.s0)) : R.n_paths;
        be.pass_begin(R);
        if constexpr (tile_hooks) { if (tiled) be.generate_tiles(job.tile_active, tiles_x); else be.generate(); }
        else be.generate();
        be.extend(0);
        be.aov(planes, off); // (walks round 0's queue: in the tile form only the slots of active sample pixels are written)
        if (samples_out) {
            if constexpr (tile_hooks) { if (tiled) be.export_aov_tiles(samples_out, off, job.tile_active, tiles_x); else be.export_aov(samples_out, off); }
            else be.export_aov(samples_out, off);
        }
        // output rows touched by the sample rows gathered: pixel row = min_y + sample row, +-2
        const int32_t f0 = band_mode ? srow0 : ps.r0, f1 = band_mode ? srow1 : ps.r1;
        const int32_t y0 = std::max(rb, g.min_y + f0 - 2), y1 = std::min(re, g.min_y + f1 - 1 + 2 + 1);
        if (ps.last_block && y1 > y0) { // ordered after the previous film launches, whichever lane ran them
            DParams Rf = R;
            if (band_mode) { Rf.row0 = srow0; Rf.row1 = srow1; Rf.n_paths = (uint32_t)band_rows * (uint32_t)g.NX; }
            if constexpr (tile_hooks) { if (tiled) be.film_aov_tiles(planes, films, y0, y1, Rf, job.tile_list, job.n_tile_list, tiles_x); else be.film_aov(planes, films, y0, y1, Rf); }
            else be.film_aov(planes, films, y0, y1, Rf);
        }
        pending[lane].active = true; pending[lane].n_paths = n_traced;
        ++pass_no;
    }
    st.ms_enqueue = std::chrono::duration<double, std::milli>(clock::now() - t_begin).count();
    for (uint32_t k = 0; k < n_lanes; ++k) finish((pass_no + k) % n_lanes);
    be.end(st);
    st.bvh_nodes = sc.n_nodes; st.bvh_max_depth = bvh_depth;
    st.ms_total = std::chrono::duration<double, std::milli>(clock::now() - t_begin).count();
    if (stats) *stats = st;
    return PTRS_OK;
}

} // namespace pt
