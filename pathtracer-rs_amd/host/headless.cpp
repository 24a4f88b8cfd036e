// ptrs_headless -- the reference's headless front-end over the HIP backend.
//
// Mirrors src/main.rs:35-145 (flag subset: SCENE, -o/--output DIR, -s/--samples, -r/--resolution WxH,
// -d/--max_depth, --default_lights, --headless; the viewer flags are accepted and ignored) and src/headless.rs:222-229
// (one-shot render, then film.to_rgba_image().save(DIR/render.png)).  Wiring follows main.rs:101-126:
//   import -> SamplerBuilder::new(spp, film.get_sample_bounds()) -> PathIntegrator::new(.., max_depth)
//   -> preprocess -> render -> save.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ptrs_host.hpp"

using namespace ptrs_host;

static bool parse_resolution(const char *s, int &w, int &h) { // main.rs:23-33
    const char *x = std::strchr(s, 'x');
    if (!x || std::strchr(x + 1, 'x')) return false;
    w = (int)std::strtof(std::string(s, x - s).c_str(), nullptr); h = (int)std::strtof(x + 1, nullptr);
    return w > 0 && h > 0;
}

int main(int argc, char **argv) {
    std::string scene_path, out_dir, dump_path, dump_full_path, env_map_path;
    bool default_lights = false, even_bands = false, preview = false, progress = false, aov = false, denoise = false, adaptive = false;
    int n_gpus = 1;
    double target_error = -1.0; int min_samples = 8; // --target_error: render until the film's error is below it, -s is then the ceiling
    int spp = 1, max_depth = 15, w = 640, h = 480; // DEFAULT_RESOLUTION common/mod.rs:14
    bool have_out = false;
    bool have_aperture = false, have_focus = false, have_focus_at = false; // the thin lens (not in the reference): they override a thinlens sensor's values
    float aperture = 0.0f, focus = 0.0f, focus_x = 0.0f, focus_y = 0.0f;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto need = [&](const char *name) -> const char * { if (i + 1 >= argc) { std::fprintf(stderr, "error: %s needs a value\n", name); std::exit(2); } return argv[++i]; };
        if (a == "-o" || a == "--output") { out_dir = need("--output"); have_out = true; }
        else if (a == "-s" || a == "--samples") spp = std::atoi(need("--samples"));
        else if (a == "-r" || a == "--resolution") { if (!parse_resolution(need("--resolution"), w, h)) { std::fprintf(stderr, "error: invalid resolution string\n"); return 2; } }
        else if (a == "-d" || a == "--max_depth") { const char *v = need("--max_depth"); char *e; long d = std::strtol(v, &e, 10); max_depth = (*e == 0) ? (int)d : 20; } // main.rs:21,87-97
        else if (a == "--dump-scene") dump_path = need("--dump-scene");
        else if (a == "--dump-scene-full") dump_full_path = need("--dump-scene-full");
        else if (a == "--default_lights") default_lights = true; // main.rs:48,99
        else if (a == "--env_map") env_map_path = need("--env_map"); // the Radiance .hdr --default_lights uses (the reference's bundled file is not shipped)
        else if (a == "--gpus") n_gpus = std::atoi(need("--gpus")); // not a flag of the reference: split the frame's rows over N devices of this process
        else if (a == "--even_bands") even_bands = true;               // equal-height bands instead of the 1-spp cost probe
        else if (a == "--preview") preview = true;                     // DIR/render.png is rewritten after every pass (the reference pushes the partial film to tev, headless.rs:197-214)
        else if (a == "--progress") progress = true;                   // a progress line per pass (the reference's progress bar, integrator.rs:631-634); like --preview it
                                                                       // renders through ptrs_render_progressive, which publishes the film after every pass (slower than the one-shot render)
        else if (a == "--aov") aov = true;                             // next to render.png: albedo.png, normal.png, depth.png (the first-hit planes of ptrs_render_aov, resolved)
        else if (a == "--denoise") denoise = true;                     // next to render.png: denoised.png (ptrs_denoise on the film and the first-hit planes, default parameters)
        else if (a == "--target_error") target_error = std::atof(need("--target_error"));  // render blocks of samples (--min_samples, then doubling, at most -s) until ptrs_film_error's
        else if (a == "--min_samples") min_samples = std::atoi(need("--min_samples"));     // largest tile error is below E (ptrs_render_converged); prints every check and the count it stopped at
        else if (a == "--adaptive") adaptive = true;                   // with --target_error: every block only on the 16 x 16 tiles still above E (ptrs_render_adaptive); writes samples.png next to render.png;
                                                                       // --aov / --denoise then take their planes from ptrs_render_aov_adaptive: every tile's planes hold the samples its film pixels hold
        else if (a == "--aperture") { aperture = std::strtof(need("--aperture"), nullptr); have_aperture = true; }  // lens radius in scene units (0: pinhole)
        else if (a == "--focus") { focus = std::strtof(need("--focus"), nullptr); have_focus = true; }             // depth of the plane in focus along the view axis
        else if (a == "--focus_at") {                                                                               // autofocus: that depth from what raster point X,Y shows (ptrs_camera_focus_distance)
            const char *v = need("--focus_at"); char *e;
            focus_x = std::strtof(v, &e);
            if (e == v || *e != ',') { std::fprintf(stderr, "error: --focus_at needs X,Y\n"); return 2; }
            const char *v2 = e + 1;
            focus_y = std::strtof(v2, &e);
            if (e == v2 || *e != 0) { std::fprintf(stderr, "error: --focus_at needs X,Y\n"); return 2; }
            have_focus_at = true;
        }
        else if (a == "--headless") {}
        else if (a == "-c" || a == "--camera" || a == "-l" || a == "--log_level" || a == "-m" || a == "--module_log" || a == "--server") (void)need(a.c_str());
        else if (!a.empty() && a[0] == '-') { std::fprintf(stderr, "error: unknown flag %s\n", a.c_str()); return 2; }
        else scene_path = a;
    }
    if (scene_path.empty() || (!have_out && dump_path.empty() && dump_full_path.empty())) {
        std::fprintf(stderr, "usage: ptrs_headless SCENE(.xml|.gltf|.glb) -o DIR [-s SPP] [-r WxH] [-d DEPTH] [--default_lights --env_map FILE.hdr] [--gpus N [--even_bands]] [--preview] [--progress] [--aov] [--denoise] [--target_error E [--min_samples N] [--adaptive]] [--aperture R] [--focus D | --focus_at X,Y] [--headless]\n");
        return 2;
    }
    if (target_error >= 0.0 && (n_gpus > 1 || preview || progress)) { std::fprintf(stderr, "error: --target_error does not combine with --gpus, --preview or --progress\n"); return 2; }
    if (have_focus && have_focus_at) { std::fprintf(stderr, "error: --focus and --focus_at exclude each other\n"); return 2; }
    if (adaptive && target_error < 0.0) { std::fprintf(stderr, "error: --adaptive needs --target_error\n"); return 2; }
    Camera camera; RenderScene scene; std::string err;
    if (!import_scene(scene_path, w, h, camera, scene, err, default_lights, env_map_path)) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 1; }
    if (!dump_full_path.empty()) { if (!dump_scene_full(dump_full_path, camera, scene)) { std::fprintf(stderr, "error: cannot write %s\n", dump_full_path.c_str()); return 1; } if (!have_out && dump_path.empty()) return 0; }
    if (!dump_path.empty()) { if (!dump_scene(dump_path, camera, scene)) { std::fprintf(stderr, "error: cannot write %s\n", dump_path.c_str()); return 1; } if (!have_out) return 0; }
    int32_t sb[4];
    camera.film.get_sample_bounds(sb);
    PathIntegrator integrator(SamplerBuilder(spp, sb), max_depth, progress || preview);
    integrator.preprocess(scene);
    if (have_aperture || have_focus || have_focus_at) {
        float r = have_aperture ? aperture : camera.lens.lens_radius, fd = have_focus ? focus : camera.lens.focal_distance;
        if (have_focus_at) {
            const int rc_f = integrator.focus_distance(camera, scene, focus_x, focus_y, fd);
            if (rc_f != PTRS_OK) { std::fprintf(stderr, "error: autofocus failed (%d): %s\n", rc_f, integrator.last_error.c_str()); return 1; }
            if (!(fd < HUGE_VALF)) { std::fprintf(stderr, "error: --focus_at %g,%g: the ray hits nothing to focus on\n", (double)focus_x, (double)focus_y); return 1; }
            std::fprintf(stderr, "INFO focus distance %.6g\n", (double)fd);
        }
        if (!camera.set_lens(r, fd)) { std::fprintf(stderr, "error: bad lens: --aperture must be finite and >= 0, and with an aperture the focus distance (--focus, --focus_at or the scene's) finite and > 0\n"); return 2; }
    }
    if (preview && have_out) integrator.on_pass = [&](uint32_t done, uint32_t total, int32_t, int32_t) {
        std::string e;
        if (done < total && !write_png_rgba8(out_dir + "/render.png", camera.film.width, camera.film.height, camera.film.to_rgba_image(), e)) std::fprintf(stderr, "\nwarning: preview: %s\n", e.c_str());
    };
    PtrsStats st{};
    std::vector<PtrsFilmPixel> planes[PTRS_AOV_PLANES];
    bool have_planes = false; // --adaptive: the planes are rendered tile by tile with the samples the film's tiles hold
    auto t0 = std::chrono::steady_clock::now();
    int rc;
    if (n_gpus > 1) {
        std::vector<PtrsStats> sts((size_t)n_gpus);
        std::vector<int32_t> bands;
        rc = integrator.render_multi(camera, scene, n_gpus, !even_bands, sts.data(), &bands);
        for (int d = 0; rc == PTRS_OK && d < n_gpus; ++d) {
            std::fprintf(stderr, "INFO device %d: rows %d..%d, %llu rays\n", d, bands[(size_t)d], bands[(size_t)d + 1], (unsigned long long)(sts[(size_t)d].rays_extension + sts[(size_t)d].rays_shadow + sts[(size_t)d].rays_mis));
            st.samples += sts[(size_t)d].samples; st.rays_extension += sts[(size_t)d].rays_extension; st.rays_shadow += sts[(size_t)d].rays_shadow; st.rays_mis += sts[(size_t)d].rays_mis;
        }
    } else if (target_error >= 0.0 && adaptive) {
        PtrsAdaptiveResult res{};
        std::vector<uint32_t> tile_spp;
        rc = integrator.render_adaptive(camera, scene, (float)target_error, (uint32_t)(min_samples < 0 ? 0 : min_samples), res, &tile_spp, &st);
        if (rc == PTRS_OK) {
            const uint32_t n_tiles = res.tiles_x * res.tiles_y;
            for (uint32_t k = 0; k < res.n_checks; ++k) std::fprintf(stderr, "INFO check %u: %u spp, %u of %u tiles active, worst %.6g\n", k + 1, res.history[k].spp, res.history[k].tiles_active, n_tiles, (double)res.history[k].max_tile_error);
            std::fprintf(stderr, "INFO stopped at %u spp (%s, target %.6g, worst tile %u)\n", res.spp_done, res.converged ? "converged" : "ceiling reached", target_error, res.worst_tile);
            // samples.png: grey = the tile's samples / the ceiling
            uint32_t ceiling = 1; while (ceiling < (uint32_t)(spp < 1 ? 1 : spp)) ceiling <<= 1; // (-s rounded up to a power of two, sobol.rs:37)
            std::vector<uint8_t> img((size_t)camera.film.width * (size_t)camera.film.height * 4);
            for (int y = 0; y < camera.film.height; ++y)
                for (int x = 0; x < camera.film.width; ++x) {
                    const uint32_t n = tile_spp[(size_t)(y / PTRS_ERROR_TILE) * res.tiles_x + (size_t)(x / PTRS_ERROR_TILE)];
                    const uint8_t g = (uint8_t)((255u * std::min(n, ceiling) + ceiling / 2u) / std::max(ceiling, 1u));
                    uint8_t *q = &img[((size_t)y * (size_t)camera.film.width + (size_t)x) * 4];
                    q[0] = q[1] = q[2] = g; q[3] = 255;
                }
            if (!write_png_rgba8(out_dir + "/samples.png", camera.film.width, camera.film.height, img, err)) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 1; }
            std::fprintf(stderr, "INFO wrote %s/samples.png\n", out_dir.c_str());
            if (aov || denoise) { // (before the sample count changes: the schedule's ceiling is -s)
                PtrsStats ast{};
                rc = integrator.render_aov_adaptive(camera, scene, (uint32_t)(min_samples < 0 ? 0 : min_samples), tile_spp, PTRS_AOV_ALBEDO | PTRS_AOV_NORMAL | PTRS_AOV_DEPTH, planes, &ast);
                if (rc != PTRS_OK) { std::fprintf(stderr, "error: aov render failed (%d): %s\n", rc, integrator.last_error.c_str()); return 1; }
                have_planes = true;
            }
            integrator.set_samples_per_pixel((int)res.spp_done);
        }
    } else if (target_error >= 0.0) {
        PtrsConvergeResult res{};
        rc = integrator.render_converged(camera, scene, (float)target_error, (uint32_t)(min_samples < 0 ? 0 : min_samples), res, &st);
        if (rc == PTRS_OK) {
            for (uint32_t k = 0; k < res.n_checks; ++k) std::fprintf(stderr, "INFO check %u: %u spp, max tile error %.6g\n", k + 1, res.history[k].spp, (double)res.history[k].max_tile_error);
            std::fprintf(stderr, "INFO stopped at %u spp (%s, target %.6g, worst tile %u)\n", res.spp_done, res.converged ? "converged" : "ceiling reached", target_error, res.worst_tile);
            integrator.set_samples_per_pixel((int)res.spp_done); // --aov / --denoise: the planes of the samples the film holds
        }
    } else rc = integrator.render(camera, scene, &st);
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc != PTRS_OK) { std::fprintf(stderr, "error: render failed (%d): %s\n", rc, integrator.last_error.c_str()); return 1; }
    std::fprintf(stderr, "INFO rendering took: %.3fs (%llu samples, %llu rays, %.1f Mray/s)\n", secs, (unsigned long long)st.samples,
                 (unsigned long long)(st.rays_extension + st.rays_shadow + st.rays_mis), (double)(st.rays_extension + st.rays_shadow + st.rays_mis) / secs / 1e6);
    const std::string out = out_dir + "/render.png"; // main.rs:70
    if (!write_png_rgba8(out, camera.film.width, camera.film.height, camera.film.to_rgba_image(), err)) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 1; }
    std::fprintf(stderr, "INFO wrote %s\n", out.c_str());
    if (aov) {
        rc = have_planes ? PTRS_OK : integrator.render_aov(camera, scene, PTRS_AOV_ALBEDO | PTRS_AOV_NORMAL | PTRS_AOV_DEPTH, planes, &st);
        if (rc != PTRS_OK) { std::fprintf(stderr, "error: aov render failed (%d): %s\n", rc, integrator.last_error.c_str()); return 1; }
        std::vector<uint8_t> img[PTRS_AOV_PLANES];
        aov_to_rgba_images(camera.film.width, camera.film.height, planes, img);
        const char *names[PTRS_AOV_PLANES] = {"/albedo.png", "/normal.png", "/depth.png"};
        for (int k = 0; k < PTRS_AOV_PLANES; ++k) {
            if (!write_png_rgba8(out_dir + names[k], camera.film.width, camera.film.height, img[k], err)) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 1; }
            std::fprintf(stderr, "INFO wrote %s%s\n", out_dir.c_str(), names[k]);
        }
    }
    if (denoise) { // (the planes of --aov, when given, are the ones the filter is guided by)
        Film dn(camera.film.width, camera.film.height);
        rc = integrator.denoise(camera, scene, planes, dn.pixels, nullptr, &st);
        if (rc != PTRS_OK) { std::fprintf(stderr, "error: denoise failed (%d): %s\n", rc, integrator.last_error.c_str()); return 1; }
        if (!write_png_rgba8(out_dir + "/denoised.png", dn.width, dn.height, dn.to_rgba_image(), err)) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 1; }
        std::fprintf(stderr, "INFO wrote %s/denoised.png (%.3f ms, %llu launches)\n", out_dir.c_str(), st.ms_total, (unsigned long long)st.kernel_launches);
    }
    return 0;
}
