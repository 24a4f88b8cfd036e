// ptrs_host.cpp -- see ptrs_host.hpp.  Plain C++17; binary32 arithmetic in the order nalgebra 0.32.2
// performs it (same order as pathtracer-rs_amd/scene.py, so both hosts emit identical bits).
#include "ptrs_host.hpp"

#include <unistd.h>
#include <zlib.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>

#include "../../include/ptrs_detmath.h"

namespace ptrs_host {

// ---- Film ------------------------------------------------------------------------------------------
void Film::clear() { for (auto &p : pixels) p = PtrsFilmPixel{{0, 0, 0}, 0}; }
void Film::get_sample_bounds(int32_t out[4]) const {
    const float r = 2.0f;
    out[0] = (int32_t)std::floor(0.5f - r); out[1] = (int32_t)std::floor(0.5f - r);
    out[2] = (int32_t)std::ceil((float)width - 0.5f + r); out[3] = (int32_t)std::ceil((float)height - 0.5f + r);
}
static float gamma_correct(float v) { return v <= 0.0031308f ? 12.92f * v : 1.055f * pt_powf(v, 1.0f / 2.4f) - 0.055f; } // math.rs:133-139
static uint8_t to_u8(float v) { // spectrum.rs:95-102: (g*255 + 0.5).clamp(0,255) as u8
    float x = gamma_correct(v) * 255.0f + 0.5f;
    if (!(x == x)) return 0; // NaN as u8 saturates to 0 in Rust
    if (x < 0.0f) x = 0.0f;
    if (x > 255.0f) x = 255.0f;
    return (uint8_t)x;
}
std::vector<uint8_t> Film::to_rgba_image() const {
    std::vector<uint8_t> out((size_t)width * height * 4);
    for (size_t i = 0; i < pixels.size(); ++i) {
        const float inv_wt = 1.0f / pixels[i].weight;
        out[4 * i] = to_u8(pixels[i].rgb[0] * inv_wt); out[4 * i + 1] = to_u8(pixels[i].rgb[1] * inv_wt);
        out[4 * i + 2] = to_u8(pixels[i].rgb[2] * inv_wt); out[4 * i + 3] = 255;
    }
    return out;
}

// ---- scene description --------------------------------------------------------------------------------
size_t RenderScene::num_triangles() const { size_t n = 0; for (auto &m : meshes) n += m.indices.size() / 3; return n; }
const PtrsSceneDesc &RenderScene::desc() {
    // Light::preprocess (light.rs:209-211,480-482) with Bounds3::bounding_sphere (bounds.rs:126-134)
    float lo[3] = {3.402823466e38f, 3.402823466e38f, 3.402823466e38f}, hi[3] = {-3.402823466e38f, -3.402823466e38f, -3.402823466e38f};
    for (auto &m : meshes) for (size_t i = 0; i < m.pos.size(); ++i) { int c = (int)(i % 3); lo[c] = std::fmin(lo[c], m.pos[i]); hi[c] = std::fmax(hi[c], m.pos[i]); }
    float center[3], d[3];
    for (int c = 0; c < 3; ++c) { center[c] = (lo[c] + hi[c]) * 0.5f; d[c] = center[c] - hi[c]; }
    const float radius = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    for (auto &l : lights) if (l.kind == PTRS_LIGHT_DIRECTIONAL || l.kind == PTRS_LIGHT_INFINITE) { std::memcpy(l.world_center, center, 12); l.world_radius = radius; }
    abi_meshes_.clear();
    for (auto &m : meshes) {
        PtrsMesh a{};
        a.n_verts = (uint32_t)(m.pos.size() / 3); a.n_tris = (uint32_t)(m.indices.size() / 3);
        a.pos = m.pos.data(); a.normal = m.normal.empty() ? nullptr : m.normal.data(); a.tangent = m.tangent.empty() ? nullptr : m.tangent.data();
        a.uv = m.uv.empty() ? nullptr : m.uv.data(); a.indices = m.indices.data();
        a.material = m.material; a.alpha_mask_tex = m.alpha_mask_tex;
        abi_meshes_.push_back(a);
    }
    desc_ = PtrsSceneDesc{};
    desc_.n_meshes = (uint32_t)abi_meshes_.size(); desc_.meshes = abi_meshes_.data();
    desc_.n_materials = (uint32_t)materials.size(); desc_.materials = materials.data();
    desc_.n_textures = (uint32_t)textures.size(); desc_.textures = textures.data();
    desc_.n_lights = (uint32_t)lights.size(); desc_.lights = lights.data();
    return desc_;
}

// ---- sampler / integrator -----------------------------------------------------------------------------
static int round_up_pow2(int v) { v -= 1; v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16; return v + 1; }
SamplerBuilder::SamplerBuilder(int spp, const int32_t bounds[4]) {
    samples_per_pixel = round_up_pow2(spp < 1 ? 1 : spp);
    if (samples_per_pixel != spp) std::fprintf(stderr, "WARN non power-of-two sample count rounded up to %d for sobol sampler\n", samples_per_pixel);
    std::memcpy(sample_bounds, bounds, 16);
    int ext = std::max(bounds[2] - bounds[0], bounds[3] - bounds[1]);
    resolution = round_up_pow2(ext);
    log_2_resolution = 31u - (uint32_t)__builtin_clz((uint32_t)resolution);
}
PathIntegrator::PathIntegrator(const SamplerBuilder &sb, int max_depth, bool show_progress_bar, int device)
    : sb_(sb), max_depth_(max_depth), show_progress_bar_(show_progress_bar), device_(device) {}
PathIntegrator::~PathIntegrator() {
    if (gpu_scene_) ptrs_scene_destroy(gpu_scene_);
    for (PtrsScene *s : multi_scenes_) if (s) ptrs_scene_destroy(s);
}
void PathIntegrator::preprocess(const RenderScene &scene) {
    if (scene.lights.size() > 16) std::fprintf(stderr, "WARN scene contains too many lights for path integrator to handle well\n");
}
PtrsRenderParams PathIntegrator::params(const Camera &camera) const {
    PtrsRenderParams p{};
    p.width = camera.film.width; p.height = camera.film.height; p.spp = sb_.samples_per_pixel; p.max_depth = max_depth_;
    p.rr_threshold = rr_threshold_; p.rr_start_depth = rr_start_depth_; p.rr_enable = rr_enable_ ? 1 : 0;
    p.row_begin = 0; p.row_end = camera.film.height; p.device = device_; p.paths_per_pass = 0; p.flags = 0;
    if (camera.lens.lens_radius > 0.0f) p.flags |= PTRS_FLAG_THIN_LENS; // &camera.abi is then read as the head of camera.lens
    return p;
}
int PathIntegrator::ensure_scene(RenderScene &scene) {
    if (!gpu_scene_ || gpu_scene_src_ != &scene) {
        if (gpu_scene_) { ptrs_scene_destroy(gpu_scene_); gpu_scene_ = nullptr; }
        int rc = ptrs_scene_create(&scene.desc(), device_, &gpu_scene_);
        if (rc != PTRS_OK) { last_error = ptrs_last_error(); return rc; }
        gpu_scene_src_ = &scene;
    }
    return PTRS_OK;
}
int PathIntegrator::render_aov(Camera &camera, RenderScene &scene, uint32_t planes, std::vector<PtrsFilmPixel> planes_inout[PTRS_AOV_PLANES], PtrsStats *stats) {
    int rc = ensure_scene(scene);
    if (rc != PTRS_OK) return rc;
    const PtrsRenderParams p = params(camera);
    const size_t npx = (size_t)camera.film.width * (size_t)camera.film.height;
    PtrsFilmPixel *ptrs[PTRS_AOV_PLANES] = {nullptr, nullptr, nullptr};
    for (uint32_t k = 0; k < PTRS_AOV_PLANES; ++k) {
        if (!(planes & (1u << k))) continue;
        if (planes_inout[k].size() != npx) planes_inout[k].assign(npx, PtrsFilmPixel{{0, 0, 0}, 0});
        ptrs[k] = planes_inout[k].data();
    }
    rc = ptrs_render_aov(gpu_scene_, &camera.abi, &p, planes, ptrs, nullptr, stats);
    if (rc != PTRS_OK) last_error = ptrs_last_error();
    return rc;
}
int PathIntegrator::denoise(Camera &camera, RenderScene &scene, std::vector<PtrsFilmPixel> planes[PTRS_AOV_PLANES], std::vector<PtrsFilmPixel> &out, const PtrsDenoiseParams *dp, PtrsStats *stats) {
    const size_t npx = (size_t)camera.film.width * (size_t)camera.film.height;
    int rc;
    if (planes[0].size() != npx || planes[1].size() != npx || planes[2].size() != npx) {
        for (int k = 0; k < PTRS_AOV_PLANES; ++k) planes[k].clear();
        if ((rc = render_aov(camera, scene, PTRS_AOV_ALBEDO | PTRS_AOV_NORMAL | PTRS_AOV_DEPTH, planes, nullptr)) != PTRS_OK) return rc;
    }
    PtrsDenoiseParams p;
    if (dp) p = *dp; else ptrs_denoise_default_params(&p);
    PtrsDenoiser *d = nullptr;
    if ((rc = ptrs_denoiser_create(device_, camera.film.width, camera.film.height, &d)) != PTRS_OK) { last_error = ptrs_last_error(); return rc; }
    out.assign(npx, PtrsFilmPixel{{0, 0, 0}, 0});
    const PtrsFilmPixel *ptrs[PTRS_AOV_PLANES] = {planes[0].data(), planes[1].data(), planes[2].data()};
    rc = ptrs_denoise(d, &p, camera.film.pixels.data(), ptrs, out.data(), stats);
    if (rc != PTRS_OK) last_error = ptrs_last_error();
    ptrs_denoiser_destroy(d);
    return rc;
}
void aov_to_rgba_images(int w, int h, const std::vector<PtrsFilmPixel> planes[PTRS_AOV_PLANES], std::vector<uint8_t> rgba_out[PTRS_AOV_PLANES]) {
    const size_t npx = (size_t)w * (size_t)h;
    const std::vector<PtrsFilmPixel> &al = planes[0], &nr = planes[1], &dp = planes[2];
    auto code = [](double v) { v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); return (uint8_t)std::floor(255.0 * v + 0.5); };
    std::vector<uint8_t> alpha(npx, 255);
    std::vector<double> depth(npx, 0.0);
    double max_depth = 0.0;
    if (dp.size() == npx)
        for (size_t i = 0; i < npx; ++i) {
            alpha[i] = dp[i].weight != 0.0f ? code((double)dp[i].rgb[1] / (double)dp[i].weight) : 0;
            depth[i] = dp[i].rgb[1] != 0.0f ? (double)dp[i].rgb[0] / (double)dp[i].rgb[1] : 0.0;
            if (depth[i] > max_depth) max_depth = depth[i];
        }
    for (int k = 0; k < PTRS_AOV_PLANES; ++k) rgba_out[k].clear();
    if (al.size() == npx) {
        rgba_out[0].resize(npx * 4);
        for (size_t i = 0; i < npx; ++i) {
            for (int c = 0; c < 3; ++c) rgba_out[0][i * 4 + c] = al[i].weight != 0.0f ? code((double)al[i].rgb[c] / (double)al[i].weight) : 0;
            rgba_out[0][i * 4 + 3] = alpha[i];
        }
    }
    if (nr.size() == npx) {
        rgba_out[1].resize(npx * 4);
        for (size_t i = 0; i < npx; ++i) {
            double n[3] = {0.0, 0.0, 0.0};
            if (nr[i].weight != 0.0f) for (int c = 0; c < 3; ++c) n[c] = (double)nr[i].rgb[c] / (double)nr[i].weight;
            const double l = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            for (int c = 0; c < 3; ++c) rgba_out[1][i * 4 + c] = code(0.5 * (l > 0.0 ? n[c] / l : 0.0) + 0.5);
            rgba_out[1][i * 4 + 3] = alpha[i];
        }
    }
    if (dp.size() == npx) {
        rgba_out[2].resize(npx * 4);
        for (size_t i = 0; i < npx; ++i) {
            const uint8_t v = max_depth > 0.0 ? code(depth[i] / max_depth) : 0;
            rgba_out[2][i * 4] = rgba_out[2][i * 4 + 1] = rgba_out[2][i * 4 + 2] = v;
            rgba_out[2][i * 4 + 3] = alpha[i];
        }
    }
}
int PathIntegrator::render(Camera &camera, RenderScene &scene, PtrsStats *stats) {
    int rc = ensure_scene(scene);
    if (rc != PTRS_OK) return rc;
    const PtrsRenderParams p = params(camera);
    if (on_pass || show_progress_bar_) { // integrator.rs:631-634 (progress bar) / headless.rs:197-214 (film read while rendering): the film is published pass by pass
        struct Ctx { PathIntegrator *self; } ctx{this};
        auto thunk = [](void *user, uint32_t done, uint32_t total, int32_t y0, int32_t y1) {
            PathIntegrator *self = static_cast<Ctx *>(user)->self;
            if (self->show_progress_bar_) std::fprintf(stderr, "\rrendering: pass %u/%u%s", done, total, done == total ? "\n" : "");
            if (self->on_pass) self->on_pass(done, total, y0, y1);
        };
        rc = ptrs_render_progressive(gpu_scene_, &camera.abi, &p, camera.film.pixels.data(), thunk, &ctx, stats);
    } else rc = ptrs_render(gpu_scene_, &camera.abi, &p, camera.film.pixels.data(), stats);
    if (rc != PTRS_OK) last_error = ptrs_last_error();
    return rc;
}
int PathIntegrator::render_converged(Camera &camera, RenderScene &scene, float target_error, uint32_t min_spp, PtrsConvergeResult &result, PtrsStats *stats) {
    int rc = ensure_scene(scene);
    if (rc != PTRS_OK) return rc;
    const PtrsRenderParams p = params(camera);
    rc = ptrs_render_converged(gpu_scene_, &camera.abi, &p, target_error, min_spp, camera.film.pixels.data(), nullptr, &result, stats);
    if (rc != PTRS_OK) last_error = ptrs_last_error();
    return rc;
}
int PathIntegrator::render_adaptive(Camera &camera, RenderScene &scene, float target_error, uint32_t min_spp, PtrsAdaptiveResult &result, std::vector<uint32_t> *tile_spp, PtrsStats *stats) {
    int rc = ensure_scene(scene);
    if (rc != PTRS_OK) return rc;
    const PtrsRenderParams p = params(camera);
    if (tile_spp) tile_spp->assign((size_t)((p.width + PTRS_ERROR_TILE - 1) / PTRS_ERROR_TILE) * (size_t)((p.height + PTRS_ERROR_TILE - 1) / PTRS_ERROR_TILE), 0u);
    rc = ptrs_render_adaptive(gpu_scene_, &camera.abi, &p, target_error, min_spp, camera.film.pixels.data(), nullptr, tile_spp ? tile_spp->data() : nullptr, &result, stats);
    if (rc != PTRS_OK) last_error = ptrs_last_error();
    return rc;
}
int PathIntegrator::render_aov_adaptive(Camera &camera, RenderScene &scene, uint32_t min_spp, const std::vector<uint32_t> &tile_spp, uint32_t planes, std::vector<PtrsFilmPixel> planes_inout[PTRS_AOV_PLANES], PtrsStats *stats) {
    int rc = ensure_scene(scene);
    if (rc != PTRS_OK) return rc;
    const PtrsRenderParams p = params(camera);
    const size_t npx = (size_t)camera.film.width * (size_t)camera.film.height;
    if (tile_spp.size() != (size_t)((p.width + PTRS_ERROR_TILE - 1) / PTRS_ERROR_TILE) * (size_t)((p.height + PTRS_ERROR_TILE - 1) / PTRS_ERROR_TILE)) { last_error = "render_aov_adaptive: tile_spp must have tiles_x * tiles_y entries"; return PTRS_ERR_INVALID; }
    PtrsFilmPixel *ptrs[PTRS_AOV_PLANES] = {nullptr, nullptr, nullptr};
    for (uint32_t k = 0; k < PTRS_AOV_PLANES; ++k) {
        if (!(planes & (1u << k))) continue;
        if (planes_inout[k].size() != npx) planes_inout[k].assign(npx, PtrsFilmPixel{{0, 0, 0}, 0});
        ptrs[k] = planes_inout[k].data();
    }
    rc = ptrs_render_aov_adaptive(gpu_scene_, &camera.abi, &p, min_spp, tile_spp.data(), planes, ptrs, stats);
    if (rc != PTRS_OK) last_error = ptrs_last_error();
    return rc;
}
int PathIntegrator::focus_distance(Camera &camera, RenderScene &scene, float raster_x, float raster_y, float &out) {
    int rc = ensure_scene(scene);
    if (rc != PTRS_OK) return rc;
    rc = ptrs_camera_focus_distance(gpu_scene_, &camera.abi, raster_x, raster_y, &out);
    if (rc != PTRS_OK) last_error = ptrs_last_error();
    return rc;
}
bool Camera::set_lens(float lens_radius, float focal_distance) {
    if (!(lens_radius >= 0.0f && std::isfinite(lens_radius))) return false;
    if (lens_radius > 0.0f && !(focal_distance > 0.0f && std::isfinite(focal_distance))) return false;
    lens.lens_radius = lens_radius; lens.focal_distance = lens_radius > 0.0f ? focal_distance : 0.0f;
    return true;
}
int PathIntegrator::render_tiles(Camera &camera, RenderScene &scene, uint32_t sample_begin, uint32_t sample_end, const std::vector<uint8_t> &tile_active, PtrsStats *stats) {
    int rc = ensure_scene(scene);
    if (rc != PTRS_OK) return rc;
    const PtrsRenderParams p = params(camera);
    if (tile_active.size() != (size_t)((p.width + PTRS_ERROR_TILE - 1) / PTRS_ERROR_TILE) * (size_t)((p.height + PTRS_ERROR_TILE - 1) / PTRS_ERROR_TILE)) { last_error = "render_tiles: one flag per 16 x 16 tile"; return PTRS_ERR_INVALID; }
    rc = ptrs_render_tiles(gpu_scene_, &camera.abi, &p, sample_begin, sample_end, tile_active.data(), camera.film.pixels.data(), nullptr, nullptr, stats);
    if (rc != PTRS_OK) last_error = ptrs_last_error();
    return rc;
}

bool probe_row_cost(PtrsScene *scene, const PtrsCamera &camera, const PtrsRenderParams &params, int /* strips: the old form's; ignored */, std::vector<float> &row_cost, std::string &err) {
    row_cost.assign((size_t)params.height, 0.0f);
    PtrsRenderParams p = params;
    p.spp = 1;
    PtrsStats st{};
    if (ptrs_render_row_cost(scene, &camera, &p, row_cost.data(), &st) != PTRS_OK) { err = ptrs_last_error(); return false; } // one 1-spp render with a device counter per sample row
    return true;
}

int PathIntegrator::render_multi(Camera &camera, RenderScene &scene, int n_devices, bool cost_weighted, PtrsStats *stats, std::vector<int32_t> *bands_out) {
    if (n_devices < 1) { last_error = "render_multi needs at least one device"; return PTRS_ERR_INVALID; }
    if (multi_src_ != &scene || (int)multi_scenes_.size() != n_devices) {
        for (PtrsScene *s : multi_scenes_) if (s) ptrs_scene_destroy(s);
        multi_scenes_.assign((size_t)n_devices, nullptr);
        for (int d = 0; d < n_devices; ++d) { // the scene is replicated: every device walks the whole BVH for its band
            int rc = ptrs_scene_create(&scene.desc(), d, &multi_scenes_[(size_t)d]);
            if (rc != PTRS_OK) { last_error = std::string("device ") + std::to_string(d) + ": " + ptrs_last_error(); return rc; }
        }
        multi_src_ = &scene; plan_key_.clear();
    }
    const PtrsRenderParams p = params(camera);
    std::vector<int32_t> bounds((size_t)n_devices + 1);
    std::vector<float> cost;
    int rc = PTRS_OK;
    if (cost_weighted && n_devices > 1) {
        // the plan of a view is made once: a second frame of the same scene, camera, resolution and depth on the same devices pays nothing
        std::string key((const char *)&camera.lens, sizeof(camera.lens));
        key.append((const char *)&p.width, sizeof(p.width)).append((const char *)&p.height, sizeof(p.height)).append((const char *)&p.max_depth, sizeof(p.max_depth)).append((const char *)&n_devices, sizeof(n_devices));
        if (key != plan_key_) {
            if (!probe_row_cost(multi_scenes_[0], camera.abi, p, 0, cost, last_error)) return PTRS_ERR_DEVICE;
            std::vector<int32_t> planned((size_t)n_devices + 1), even((size_t)n_devices + 1);
            if ((rc = ptrs_plan_bands(p.height, (uint32_t)n_devices, cost.data(), planned.data())) != PTRS_OK || (rc = ptrs_plan_bands(p.height, (uint32_t)n_devices, nullptr, even.data())) != PTRS_OK) { last_error = ptrs_last_error(); return rc; }
            auto worst = [&](const std::vector<int32_t> &b) { double w = 0.0; for (int d = 0; d < n_devices; ++d) { double c = 0.0; for (int32_t y = b[(size_t)d]; y < b[(size_t)d + 1]; ++y) c += cost[(size_t)y]; w = std::max(w, c); } return w; };
            plan_ = worst(even) > 1.01 * worst(planned) ? planned : even; // equal bands unless the plan takes at least 1 % off the slowest band
            plan_key_ = key;
        }
        bounds = plan_;
    } else if ((rc = ptrs_plan_bands(p.height, (uint32_t)n_devices, nullptr, bounds.data())) != PTRS_OK) { last_error = ptrs_last_error(); return rc; }
    if (bands_out) *bands_out = bounds;
    rc = ptrs_render_multi(multi_scenes_.data(), (uint32_t)n_devices, &camera.abi, &p, bounds.data(), camera.film.pixels.data(), stats);
    if (rc != PTRS_OK) last_error = ptrs_last_error();
    return rc;
}

// ---- minimal XML ------------------------------------------------------------------------------------------
struct Node {
    std::string name;
    std::map<std::string, std::string> attr;
    std::vector<std::unique_ptr<Node>> kids;
    const Node *child(const std::string &n) const { for (auto &k : kids) if (k->name == n) return k.get(); return nullptr; }
    const Node *child_named(const std::string &n, const std::string &name_attr) const {
        for (auto &k : kids) if (k->name == n) { auto it = k->attr.find("name"); if (it != k->attr.end() && it->second == name_attr) return k.get(); }
        return nullptr;
    }
    std::string get(const std::string &a, const std::string &def = "") const { auto it = attr.find(a); return it == attr.end() ? def : it->second; }
};
struct Parser {
    const std::string &s; size_t i = 0; std::string err;
    explicit Parser(const std::string &src) : s(src) {}
    void ws() { while (i < s.size() && std::isspace((unsigned char)s[i])) ++i; }
    bool skip_misc() { // comments, declarations, text
        for (;;) {
            while (i < s.size() && s[i] != '<') ++i;
            if (i >= s.size()) return false;
            if (s.compare(i, 4, "<!--") == 0) { size_t e = s.find("-->", i); if (e == std::string::npos) return false; i = e + 3; continue; }
            if (s.compare(i, 2, "<?") == 0) { size_t e = s.find("?>", i); if (e == std::string::npos) return false; i = e + 2; continue; }
            return true;
        }
    }
    std::unique_ptr<Node> element() {
        if (!skip_misc() || s[i] != '<' || s[i + 1] == '/') return nullptr;
        ++i;
        auto n = std::make_unique<Node>();
        while (i < s.size() && !std::isspace((unsigned char)s[i]) && s[i] != '>' && s[i] != '/') n->name += s[i++];
        for (;;) {
            ws();
            if (i >= s.size()) { err = "unexpected end of file"; return nullptr; }
            if (s[i] == '/') { i += 2; return n; } // "/>"
            if (s[i] == '>') { ++i; break; }
            std::string key;
            while (i < s.size() && s[i] != '=' && !std::isspace((unsigned char)s[i])) key += s[i++];
            ws(); if (s[i] != '=') { err = "attribute without value"; return nullptr; }
            ++i; ws();
            char q = s[i++];
            std::string val;
            while (i < s.size() && s[i] != q) val += s[i++];
            ++i;
            n->attr[key] = val;
        }
        for (;;) {
            if (!skip_misc()) { err = "unterminated element " + n->name; return nullptr; }
            if (s[i + 1] == '/') { size_t e = s.find('>', i); i = e + 1; return n; }
            auto k = element();
            if (!k) return nullptr;
            n->kids.push_back(std::move(k));
        }
    }
};

// ---- Mitsuba import -----------------------------------------------------------------------------------------
static std::vector<float> parse_floats(const std::string &v) {
    std::vector<float> out; std::string t = v;
    for (auto &c : t) if (c == ',') c = ' ';
    std::istringstream is(t); std::string tok;
    while (is >> tok) out.push_back(std::strtof(tok.c_str(), nullptr)); // Rust str::parse::<f32>: correctly rounded, like strtof
    return out;
}
static void transform_point(const float m[16], const float p[3], float out[3]) { for (int r = 0; r < 3; ++r) out[r] = ((m[4 * r] * p[0] + m[4 * r + 1] * p[1]) + m[4 * r + 2] * p[2]) + m[4 * r + 3]; }
static void transform_vector(const float m[16], const float v[3], float out[3]) { for (int r = 0; r < 3; ++r) out[r] = (m[4 * r] * v[0] + m[4 * r + 1] * v[1]) + m[4 * r + 2] * v[2]; }

static int32_t add_const_tex(RenderScene &s, int channels, float a, float b, float c) {
    PtrsTexture t{}; t.kind = PTRS_TEX_CONSTANT; t.channels = channels; t.value[0] = a; t.value[1] = b; t.value[2] = c; t.su = t.sv = 1.0f;
    s.textures.push_back(t);
    return (int32_t)s.textures.size() - 1;
}
static int32_t add_material(RenderScene &s, int kind, std::initializer_list<int32_t> tex, int flags = 0) {
    PtrsMaterial m{}; m.kind = kind; m.flags = flags; m.inner = -1;
    for (int k = 0; k < 6; ++k) m.tex[k] = -1;
    int k = 0; for (int32_t t : tex) m.tex[k++] = t;
    s.materials.push_back(m);
    return (int32_t)s.materials.size() - 1;
}
// heck SnakeCase: a word starts at an upper-case letter after a lower-case one, and at the last letter of an upper-case run that a
// lower-case letter follows (intIOR -> int_ior, diffuseReflectance -> diffuse_reflectance)
static std::string snake(const std::string &s) {
    std::string o; int mode = 0; // case of the last letter seen: 1 lower, 2 upper
    for (size_t i = 0; i < s.size(); ++i) {
        const unsigned char c = (unsigned char)s[i];
        if (std::isupper(c)) {
            const bool next_lower = i + 1 < s.size() && std::islower((unsigned char)s[i + 1]);
            if (!o.empty() && o.back() != '_' && (mode == 1 || (mode == 2 && next_lower))) o += '_';
            o += (char)std::tolower(c); mode = 2;
        } else { o += (char)c; if (std::islower(c)) mode = 1; }
    }
    return o;
}

static bool rgb_of(const Node &n, float out[3], std::string &err) {
    auto v = parse_floats(n.get("value"));
    if (v.size() < 3) { err = "rgb parameter " + n.get("name") + " needs three values"; return false; }
    out[0] = v[0]; out[1] = v[1]; out[2] = v[2];
    return true;
}

// texture_from_mitsuba, pathtracer/importer/mitsuba.rs:24-67
static int32_t texture_from_mitsuba(RenderScene &s, const Node &el, const std::string &base, std::string &err) {
    const std::string kind = el.get("type");
    if (kind == "checkerboard") {
        std::map<std::string, const Node *> rgbs, floats;
        for (auto &k : el.kids) { if (k->name == "rgb") rgbs[snake(k->get("name"))] = k.get(); if (k->name == "float") floats[snake(k->get("name"))] = k.get(); }
        for (const char *name : {"color0", "color1"}) if (!rgbs.count(name)) { err = std::string("checkerboard texture without ") + name; return -1; }
        for (const char *name : {"uscale", "vscale", "uoffset", "voffset"}) if (!floats.count(name)) { err = std::string("checkerboard texture without ") + name; return -1; }
        PtrsTexture t{}; t.kind = PTRS_TEX_CHECKER; t.channels = 3; t.wrap = PTRS_WRAP_REPEAT;
        if (!rgb_of(*rgbs["color0"], t.value, err) || !rgb_of(*rgbs["color1"], t.value2, err)) return -1;
        auto f = [&](const char *name) { return std::strtof(floats[name]->get("value").c_str(), nullptr); };
        t.su = f("uscale"); t.sv = f("vscale"); t.du = f("uoffset"); t.dv = f("voffset");
        s.textures.push_back(t);
        return (int32_t)s.textures.size() - 1;
    }
    if (kind == "bitmap") {
        const Node *fn = el.child_named("string", "filename");
        if (!fn) { err = "bitmap texture without filename"; return -1; }
        int rows, cols; std::vector<uint8_t> rgb;
        if (!load_rgb8_image(base + "/" + fn->get("value"), rows, cols, rgb, err)) return -1;
        const float uvmap[4] = {1.0f, -1.0f, 0.0f, 0.0f}; // the reference's own TODO: "verify that this -1 on the v is actually a feature of mitsuba"
        return add_spectrum_image_texture(s, rgb, rows, cols, PTRS_WRAP_REPEAT, uvmap);
    }
    err = "unsupported texture type " + kind;
    return -1;
}

// material_from_bsdf, pathtracer/importer/mitsuba.rs:84-181
static int32_t material_from_bsdf(RenderScene &s, const Node &el, const std::string &base, std::string &err) {
    const std::string kind = el.get("type");
    std::map<std::string, std::vector<float>> rgbs; std::map<std::string, float> floats;
    for (auto &k : el.kids) {
        if (k->name == "rgb") { float c[3]; if (!rgb_of(*k, c, err)) return -1; rgbs[k->get("name")] = {c[0], c[1], c[2]}; }
        if (k->name == "float") floats[snake(k->get("name"))] = std::strtof(k->get("value").c_str(), nullptr);
    }
    const Node *texture = el.child("texture");
    // texture_with_defaults (mitsuba.rs:69-82): texture, else rgb, else 1
    auto with_defaults = [&](const char *a, const char *b) -> int32_t {
        if (texture) return texture_from_mitsuba(s, *texture, base, err);
        std::vector<float> c = {1.0f, 1.0f, 1.0f};
        if (rgbs.count(a)) c = rgbs[a]; else if (b && rgbs.count(b)) c = rgbs[b];
        return add_const_tex(s, 3, c[0], c[1], c[2]);
    };
    if (kind == "twosided") { const Node *in = el.child("bsdf"); if (!in) { err = "twosided without bsdf"; return -1; } return material_from_bsdf(s, *in, base, err); }
    if (kind == "diffuse") { int32_t t0 = with_defaults("reflectance", nullptr); if (t0 < 0) return -1; return add_material(s, PTRS_MAT_MATTE, {t0}); }
    if (kind == "conductor" || kind == "roughconductor") {
        const Node *mat = el.child_named("string", "material");
        if (kind == "conductor" && mat) { if (mat->get("value") == "none") return add_material(s, PTRS_MAT_MIRROR, {}); err = "other material values not supported yet!"; return -1; }
        if (!rgbs.count("eta") || !rgbs.count("k")) { err = "conductor without eta/k"; return -1; }
        if (kind == "roughconductor" && !floats.count("alpha")) { err = "roughconductor without alpha"; return -1; }
        auto e = rgbs["eta"], k = rgbs["k"];
        float alpha = kind == "conductor" ? 0.001f : floats["alpha"];
        int32_t t0 = add_const_tex(s, 3, e[0], e[1], e[2]), t1 = add_const_tex(s, 3, k[0], k[1], k[2]);
        int32_t t2 = with_defaults("specularReflectance", "specular_reflectance"); if (t2 < 0) return -1;
        int32_t t3 = add_const_tex(s, 1, alpha, 0, 0);
        return add_material(s, PTRS_MAT_METAL, {t0, t1, t2, t3, -1, -1}, 0);
    }
    if (kind == "dielectric") {
        if (!floats.count("int_ior")) { err = "dielectric without intIOR"; return -1; }
        int32_t t0 = add_const_tex(s, 3, 1, 1, 1), t1 = add_const_tex(s, 3, 1, 1, 1), t2 = add_const_tex(s, 1, floats["int_ior"], 0, 0);
        return add_material(s, PTRS_MAT_GLASS, {t0, t1, t2});
    }
    if (kind == "plastic" || kind == "roughplastic") {
        if (!floats.count("int_ior") || (kind == "roughplastic" && !floats.count("alpha"))) { err = kind + " without intIOR / alpha"; return -1; }
        float e = floats["int_ior"];
        float r0 = ((e - 1.0f) * (e - 1.0f)) / ((e + 1.0f) * (e + 1.0f));
        float a = kind == "plastic" ? 0.001f : floats["alpha"];
        int32_t t0 = with_defaults("diffuseReflectance", "diffuse_reflectance"); if (t0 < 0) return -1;
        int32_t t1 = add_const_tex(s, 3, r0, r0, r0), t2 = add_const_tex(s, 1, a, 0, 0), t3 = add_const_tex(s, 1, a, 0, 0);
        return add_material(s, PTRS_MAT_SUBSTRATE, {t0, t1, t2, t3}, 0);
    }
    err = "unsupported bsdf type " + kind;
    return -1;
}

// genmesh 0.6.2 Plane::new / Cube::new (restated from memory)
static void gen_rectangle(std::vector<float> &pos, std::vector<float> &nrm, std::vector<uint32_t> &idx) {
    pos = {-1, -1, 0, 1, -1, 0, -1, 1, 0, 1, 1, 0};
    nrm = {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1};
    idx = {0, 1, 3, 0, 3, 2};
}
static void gen_cube(std::vector<float> &pos, std::vector<float> &nrm, std::vector<uint32_t> &idx) {
    static const float N[6][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
    static const int Q[6][4] = {{6, 7, 5, 4}, {0, 1, 3, 2}, {3, 7, 6, 2}, {4, 5, 1, 0}, {5, 7, 3, 1}, {0, 2, 6, 4}};
    pos.clear(); nrm.clear(); idx.clear();
    for (int f = 0; f < 6; ++f) {
        for (int v = 0; v < 4; ++v) {
            int id = Q[f][v];
            pos.push_back(id & 4 ? 1.0f : -1.0f); pos.push_back(id & 2 ? 1.0f : -1.0f); pos.push_back(id & 1 ? 1.0f : -1.0f);
            nrm.push_back(N[f][0]); nrm.push_back(N[f][1]); nrm.push_back(N[f][2]);
        }
        uint32_t b = 4u * f;
        idx.insert(idx.end(), {b, b + 1, b + 2, b, b + 2, b + 3});
    }
}

// genmesh 0.6.2 SphereUv::new(10, 10) under Similarity3(center, no rotation, radius) (common/importer/mitsuba.rs:60-79; restated from
// memory): pole, 9 rings of 10, pole; 10 triangles, 80 quads as (x,y,z),(x,z,w), 10 triangles.  The normal is the unit vertex.
static void gen_sphere(const float center[3], float radius, std::vector<float> &pos, std::vector<float> &nrm, std::vector<uint32_t> &idx) {
    const int su = 10, sv = 10;
    const float PI = 3.14159274101257324f;
    pos.clear(); nrm.clear(); idx.clear();
    auto vert = [&](int u, int v) {
        const float a = ((float)u / (float)su) * PI * 2.0f, b = ((float)v / (float)sv) * PI;
        const float ca = (float)std::cos((double)a), sa = (float)std::sin((double)a), cb = (float)std::cos((double)b), sb = (float)std::sin((double)b);
        const float n[3] = {ca * sb, sa * sb, cb};
        for (int c = 0; c < 3; ++c) { nrm.push_back(n[c]); pos.push_back(n[c] * radius + center[c]); }
    };
    vert(0, 0);
    for (int v = 1; v < sv; ++v) for (int u = 0; u < su; ++u) vert(u, v);
    vert(0, sv);
    auto f = [&](int u, int v) -> uint32_t { return v == 0 ? 0u : v == sv ? (uint32_t)((sv - 1) * su + 1) : (uint32_t)((v - 1) * su + (u % su) + 1); };
    for (int v = 0; v < sv; ++v) for (int u = 0; u < su; ++u) {
        if (v == 0) idx.insert(idx.end(), {f(u, v), f(u, v + 1), f(u + 1, v + 1)});
        else if (v == sv - 1) idx.insert(idx.end(), {f(u + 1, v + 1), f(u + 1, v), f(u, v)});
        else { const uint32_t x = f(u, v), y = f(u, v + 1), z = f(u + 1, v + 1), w = f(u + 1, v); idx.insert(idx.end(), {x, y, z, x, z, w}); }
    }
}

// load_obj (common/importer/mitsuba.rs:81-151): the v / vn / vt lists in file order and the triangles; one object, one geometry,
// triangles only, normals required, position = normal = texture index at every corner.  Values are parsed as binary64 and narrowed.
static bool load_obj(const std::string &path, std::vector<float> &pos, std::vector<float> &nrm, std::vector<float> &uv, std::vector<uint32_t> &idx, std::string &err) {
    std::ifstream f(path);
    if (!f) { err = "cannot open " + path; return false; }
    auto fail = [&](const std::string &rule) { err = path + ": " + rule; return false; };
    pos.clear(); nrm.clear(); uv.clear(); idx.clear();
    std::vector<long> raw;
    int n_obj = 0, n_mtl = 0;
    std::string line;
    while (std::getline(f, line)) {
        const std::string body = line.substr(0, line.find('#'));
        std::istringstream is(body); std::vector<std::string> tok; std::string t;
        while (is >> t) tok.push_back(t);
        if (tok.empty()) continue;
        const std::string &key = tok[0]; const size_t na = tok.size() - 1;
        auto malformed = [&]() { size_t a = line.find_first_not_of(" \t\r\n"), b = line.find_last_not_of(" \t\r\n"); return fail("malformed line: " + (a == std::string::npos ? std::string() : line.substr(a, b - a + 1))); };
        auto floats = [&](size_t n, std::vector<float> &out) { for (size_t k = 1; k <= n; ++k) { char *e; const double v = std::strtod(tok[k].c_str(), &e); if (e == tok[k].c_str() || *e) return false; out.push_back((float)v); } return true; };
        if (key == "v") { if (na < 3) return fail("v needs three coordinates"); if (!floats(3, pos)) return malformed(); }
        else if (key == "vn") { if (na < 3) return fail("vn needs three coordinates"); if (!floats(3, nrm)) return malformed(); }
        else if (key == "vt") { if (na < 2) return fail("vt needs two coordinates"); if (!floats(2, uv)) return malformed(); }
        else if (key == "f") {
            if (na != 3) return fail("only triangle faces are supported");
            for (size_t k = 1; k <= 3; ++k) {
                std::vector<std::string> parts; size_t a = 0;
                for (;;) { const size_t b = tok[k].find('/', a); parts.push_back(tok[k].substr(a, b == std::string::npos ? b : b - a)); if (b == std::string::npos) break; a = b + 1; }
                long v[3] = {0, 0, 0}; bool have[3] = {false, false, false};
                for (size_t c = 0; c < parts.size() && c < 3; ++c) { if (parts[c].empty()) { if (c == 0) return malformed(); continue; } char *e; v[c] = std::strtol(parts[c].c_str(), &e, 10); if (*e) return malformed(); have[c] = true; }
                if (!have[2]) return fail("faces need normals (v/vt/vn or v//vn)");
                if (v[0] != v[2]) return fail("position and normal index must be equal");
                if (have[1] && v[0] != v[1]) return fail("position and texture index must be equal");
                raw.push_back(v[0] > 0 ? v[0] : (long)(pos.size() / 3) + 1 + v[0]);
            }
        }
        else if (key == "o") { if (++n_obj > 1) return fail("only one object is supported"); }
        else if (key == "usemtl") { if (++n_mtl > 1) return fail("only one geometry (usemtl) per object is supported"); }
        else if (key == "g" || key == "s" || key == "mtllib") {}
        else return fail("unsupported statement " + key);
    }
    if (raw.empty()) return fail("no faces");
    if (nrm.size() != pos.size()) return fail("normal count must equal vertex count");
    if (!uv.empty() && uv.size() / 2 != pos.size() / 3) return fail("texture coordinate count must equal vertex count");
    for (long v : raw) { if (v < 1 || v > (long)(pos.size() / 3)) return fail("face index out of range"); idx.push_back((uint32_t)(v - 1)); }
    return true;
}

// Matrix4::from_euler_angles(-pi/2, -pi/2, 0).append_nonuniform_scaling((1, 1, -1)) (pathtracer/importer/mitsuba.rs:365-372):
// Rz(yaw) Ry(pitch) Rx(roll) written out as nalgebra does, then the ROWS scaled.  [[0,1,0],[0,0,1],[-1,0,0]] for exact angles.
static void env_light_to_world(float m[16]) {
    const float h = (float)(-3.14159265358979323846 / 2.0); // -f32::consts::FRAC_PI_2
    const float sr = (float)std::sin((double)h), cr = (float)std::cos((double)h), sp = sr, cp = cr, sy = 0.0f, cy = 1.0f;
    const float e[16] = {cy * cp, (cy * sp) * sr - sy * cr, (cy * sp) * cr + sy * sr, 0,
                         sy * cp, (sy * sp) * sr + cy * cr, (sy * sp) * cr - cy * sr, 0,
                         -sp, cp * sr, cp * cr, 0, 0, 0, 0, 1};
    const float sc[3] = {1.0f, 1.0f, -1.0f};
    std::memcpy(m, e, 64);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) m[4 * r + c] = m[4 * r + c] * sc[r];
}

static std::string default_env_map_path() { // the reference reads it from its source tree (CARGO_MANIFEST_DIR/data)
    const char *name = "data/abandoned_tank_farm_04_1k.hdr";
    char buf[4096]; const ssize_t n = readlink("/proc/self/exe", buf, sizeof(buf) - 1);
    if (n > 0) {
        std::string exe(buf, (size_t)n); const size_t k = exe.find_last_of('/');
        const std::string p = (k == std::string::npos ? std::string(".") : exe.substr(0, k)) + "/../" + name;
        if (std::ifstream(p)) return p;
    }
    return name;
}

// get_camera (common/importer/mitsuba.rs:685-710, Q30) + Camera::new (common/mod.rs:33-62)
static void make_camera(const float cam_to_world[16], float fov_deg, int film_w, int film_h, int res_w, int res_h, Camera &cam) {
    const float PI = 3.14159274101257324f;
    const float fov = fov_deg * (float)(3.14159265358979323846 / 180.0); // f32::to_radians
    // Rotation3::new((0,-pi,0)) = from_axis_angle(normalize, |.|)
    float a[3] = {0.0f, -PI, 0.0f};
    float angle = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    float ux = a[0] / angle, uy = a[1] / angle, uz = a[2] / angle;
    float sn = (float)std::sin((double)angle), cs = (float)std::cos((double)angle), omc = 1.0f - cs;
    float sqx = ux * ux, sqy = uy * uy, sqz = uz * uz;
    float R[16] = {sqx + (1.0f - sqx) * cs, ux * uy * omc - uz * sn, ux * uz * omc + uy * sn, 0,
                   ux * uy * omc + uz * sn, sqy + (1.0f - sqy) * cs, uy * uz * omc - ux * sn, 0,
                   ux * uz * omc - uy * sn, uy * uz * omc + ux * sn, sqz + (1.0f - sqz) * cs, 0, 0, 0, 0, 1};
    float M[16];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { float acc = 0.0f; for (int k = 0; k < 4; ++k) acc = acc + cam_to_world[4 * i + k] * R[4 * k + j]; M[4 * i + j] = acc; }
    // try_convert::<Projective3, Similarity3>: normalise columns; scale forced to 1
    float r[3][3];
    for (int c = 0; c < 3; ++c) {
        float x = M[c], y = M[4 + c], z = M[8 + c];
        float n = std::sqrt((x * x + y * y) + z * z);
        r[0][c] = x / n; r[1][c] = y / n; r[2][c] = z / n;
    }
    // UnitQuaternion::from_rotation_matrix
    float tr = (r[0][0] + r[1][1]) + r[2][2], q = 0.25f, w, i, j, k;
    if (tr > 0.0f) { float d = std::sqrt(tr + 1.0f) * 2.0f; w = q * d; i = (r[2][1] - r[1][2]) / d; j = (r[0][2] - r[2][0]) / d; k = (r[1][0] - r[0][1]) / d; }
    else if (r[0][0] > r[1][1] && r[0][0] > r[2][2]) { float d = std::sqrt(((1.0f + r[0][0]) - r[1][1]) - r[2][2]) * 2.0f; w = (r[2][1] - r[1][2]) / d; i = q * d; j = (r[0][1] + r[1][0]) / d; k = (r[0][2] + r[2][0]) / d; }
    else if (r[1][1] > r[2][2]) { float d = std::sqrt(((1.0f + r[1][1]) - r[0][0]) - r[2][2]) * 2.0f; w = (r[0][2] - r[2][0]) / d; i = (r[0][1] + r[1][0]) / d; j = q * d; k = (r[1][2] + r[2][1]) / d; }
    else { float d = std::sqrt(((1.0f + r[2][2]) - r[0][0]) - r[1][1]) * 2.0f; w = (r[1][0] - r[0][1]) / d; i = (r[0][2] + r[2][0]) / d; j = (r[1][2] + r[2][1]) / d; k = q * d; }
    const float rot[4] = {i, j, k, w}, trans[3] = {M[3], M[7], M[11]};
    make_camera_perspective(rot, trans, (float)res_w / (float)res_h, fov * ((float)film_h / (float)film_w), 0.01f, 10000.0f, res_w, res_h, cam);
}

void make_camera_perspective(const float rot[4], const float trans[3], float aspect, float fovy, float zn, float zf, int res_w, int res_h, Camera &cam) {
    PtrsCamera &c = cam.abi;
    std::memcpy(c.rot, rot, 16); std::memcpy(c.trans, trans, 12);
    const float W = (float)res_w, H = (float)res_h;
    c.m11 = 1.0f / (float)std::tan((double)(fovy / 2.0f));
    c.m00 = c.m11 / aspect;
    c.m22 = (zf + zn) / (zn - zf);
    c.m23 = zf * zn * 2.0f / (zn - zf);
    const float sx = W * 0.5f, sy = H * -0.5f, ax = 1.0f / sx, by = 1.0f / sy;
    const float r2s[16] = {ax, 0, 0, -1.0f, 0, by, 0, 1.0f, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(c.raster_to_screen, r2s, 64);
    const float n = c.m22 / c.m23, inv00 = 1.0f / c.m00, inv11 = 1.0f / c.m11;
    const float p0[3] = {(inv00 * -1.0f) / n, (inv11 * 1.0f) / n, -1.0f / n};
    const float px[3] = {(inv00 * ax + inv00 * -1.0f) / n, (inv11 * 1.0f) / n, -1.0f / n};
    const float py[3] = {(inv00 * -1.0f) / n, (inv11 * by + inv11 * 1.0f) / n, -1.0f / n};
    for (int t = 0; t < 3; ++t) { c.dx_camera[t] = px[t] - p0[t]; c.dy_camera[t] = py[t] - p0[t]; }
    cam.film = Film(res_w, res_h);
}

bool import_scene(const std::string &path, int res_w, int res_h, Camera &camera, RenderScene &scene, std::string &err, bool default_lights, const std::string &env_map_path) {
    const size_t dot = path.rfind('.');
    const std::string ext = dot == std::string::npos ? "" : path.substr(dot);
    if (ext == ".gltf" || ext == ".glb") return import_gltf(path, res_w, res_h, default_lights, env_map_path, camera, scene, err); // importer/mod.rs:17-18
    if (ext != ".xml") { err = "unsupported format!"; return false; } // importer/mod.rs:15-23
    std::ifstream f(path, std::ios::binary);
    if (!f) { err = "cannot open " + path; return false; }
    std::string src((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    Parser P(src);
    auto root = P.element();
    if (!root || root->name != "scene") { err = "not a mitsuba scene: " + P.err; return false; }
    const Node *sensor = root->child("sensor");
    if (!sensor) { err = "scene without sensor"; return false; }
    const Node *fovn = sensor->child_named("float", "fov"), *film = sensor->child("film"), *tf = sensor->child("transform");
    if (!fovn || !film || !tf || !tf->child("matrix")) { err = "sensor needs fov, film and toWorld matrix"; return false; }
    const Node *fw = film->child_named("integer", "width"), *fh = film->child_named("integer", "height");
    if (!fw || !fh) { err = "film needs width and height"; return false; }
    auto cm = parse_floats(tf->child("matrix")->get("value"));
    if (cm.size() != 16) { err = "camera matrix needs 16 values"; return false; }
    make_camera(cm.data(), std::strtof(fovn->get("value").c_str(), nullptr), std::atoi(fw->get("value").c_str()), std::atoi(fh->get("value").c_str()), res_w, res_h, camera);
    camera.set_lens(0.0f, 0.0f);
    if (sensor->get("type") == "thinlens") { // Mitsuba's thin-lens sensor: aperture_radius, focus_distance
        const Node *ap = sensor->child_named("float", "aperture_radius"), *fd = sensor->child_named("float", "focus_distance");
        if (!ap || !fd) { err = "thinlens sensor: aperture_radius and focus_distance are required"; return false; }
        if (!camera.set_lens(std::strtof(ap->get("value").c_str(), nullptr), std::strtof(fd->get("value").c_str(), nullptr))) { err = "thinlens sensor: aperture_radius must be finite and >= 0, focus_distance finite and > 0"; return false; }
    }
    scene = RenderScene();
    const size_t slash = path.find_last_of('/');
    const std::string base = slash == std::string::npos ? "." : path.substr(0, slash);
    std::map<std::string, int32_t> named;
    for (auto &k : root->kids) if (k->name == "bsdf") { int32_t m = material_from_bsdf(scene, *k, base, err); if (m < 0) return false; named[k->get("id")] = m; }
    for (auto &k : root->kids) {
        if (k->name != "shape") continue;
        std::vector<float> pos, nrm, uv; std::vector<uint32_t> idx;
        const std::string kind = k->get("type");
        float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        if (const Node *t = k->child("transform")) if (const Node *mn = t->child("matrix")) { auto v = parse_floats(mn->get("value")); if (v.size() != 16) { err = "shape matrix needs 16 values"; return false; } std::memcpy(M, v.data(), 64); }
        if (kind == "rectangle") gen_rectangle(pos, nrm, idx);
        else if (kind == "cube") gen_cube(pos, nrm, idx);
        else if (kind == "sphere") {
            const Node *pt = k->child("point"), *rad = k->child("float");
            if (!pt || !rad) { err = "sphere needs a center point and a radius"; return false; }
            const float c[3] = {std::strtof(pt->get("x").c_str(), nullptr), std::strtof(pt->get("y").c_str(), nullptr), std::strtof(pt->get("z").c_str(), nullptr)};
            gen_sphere(c, std::strtof(rad->get("value").c_str(), nullptr), pos, nrm, idx);
            const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            std::memcpy(M, I, 64); // Shape::Sphere has no transform: obj_to_world stays the identity
        } else if (kind == "obj") {
            const Node *fn = k->child("string");
            if (!fn) { err = "obj shape without filename"; return false; }
            if (!load_obj(base + "/" + fn->get("value"), pos, nrm, uv, idx, err)) return false;
            if (const Node *b = k->child("boolean")) if (b->get("value") == "true") { std::fprintf(stderr, "WARN face normals on for obj, vertex normals will be disregarded\n"); nrm.clear(); }
        } else { err = "unsupported shape type " + kind; return false; }
        Mesh mesh; mesh.pos.resize(pos.size()); mesh.normal.resize(nrm.size()); mesh.uv = uv; mesh.indices = idx;
        for (size_t v = 0; v < pos.size() / 3; ++v) transform_point(M, &pos[3 * v], &mesh.pos[3 * v]);
        for (size_t v = 0; v < nrm.size() / 3; ++v) transform_vector(M, &nrm[3 * v], &mesh.normal[3 * v]); // Q15
        if (const Node *ref = k->child("ref")) { auto it = named.find(ref->get("id")); if (it == named.end()) { err = "unknown bsdf id " + ref->get("id"); return false; } mesh.material = it->second; }
        else if (const Node *b = k->child("bsdf")) { mesh.material = material_from_bsdf(scene, *b, base, err); if (mesh.material < 0) return false; }
        else { err = "either ref exists or embedded bsdf exists"; return false; }
        const uint32_t mi = (uint32_t)scene.meshes.size();
        if (const Node *em = k->child("emitter")) if (em->get("type") == "area") { // one DiffuseAreaLight per triangle (mitsuba.rs:306-323)
            const Node *rad = em->child("rgb");
            float c[3] = {1, 1, 1};
            if (rad && !rgb_of(*rad, c, err)) return false;
            int32_t ke = add_const_tex(scene, 3, c[0], c[1], c[2]);
            for (uint32_t t = 0; t < idx.size() / 3; ++t) { PtrsLight L{}; L.kind = PTRS_LIGHT_AREA; L.mesh = mi; L.tri = t; L.ke_tex = ke; L.lmap_tex = -1; scene.lights.push_back(L); }
        }
        scene.meshes.push_back(std::move(mesh));
    }
    // scene-level emitters join the list after every shape's area lights, in document order (mitsuba.rs:374-420)
    for (auto &k : root->kids) {
        if (k->name != "emitter") continue;
        const std::string kind = k->get("type");
        float E[16]; env_light_to_world(E);
        if (kind == "area") std::fprintf(stderr, "WARN area lights should not be standalone!\n");
        else if (kind == "point") {}
        else if (kind == "envmap") {
            const Node *fn = k->child("string"), *t = k->child("transform"), *mn = t ? t->child("matrix") : nullptr;
            if (!fn || !mn) { err = "envmap emitter needs a toWorld matrix and a filename"; return false; }
            auto v = parse_floats(mn->get("value"));
            if (v.size() != 16) { err = "envmap matrix needs 16 values"; return false; }
            float L2W[16]; matmul4(v.data(), E, L2W);
            if (!add_env_light_from_file(scene, base + "/" + fn->get("value"), L2W, err)) return false;
        } else if (kind == "sunsky") {
            std::fprintf(stderr, "WARN sunsky emitter not supported, putting default env map instead\n");
            if (!add_env_light_from_file(scene, env_map_path.empty() ? default_env_map_path() : env_map_path, E, err)) return false;
        } else { err = "unsupported emitter type " + kind; return false; }
    }
    return true;
}

// ---- PNG (zlib) ---------------------------------------------------------------------------------------------
bool write_png_rgba8(const std::string &path, int w, int h, const std::vector<uint8_t> &rgba, std::string &err) {
    std::vector<uint8_t> raw((size_t)h * ((size_t)w * 4 + 1));
    for (int y = 0; y < h; ++y) { raw[(size_t)y * (w * 4 + 1)] = 0; std::memcpy(&raw[(size_t)y * (w * 4 + 1) + 1], &rgba[(size_t)y * w * 4], (size_t)w * 4); }
    uLongf clen = compressBound((uLong)raw.size());
    std::vector<uint8_t> comp(clen);
    if (compress2(comp.data(), &clen, raw.data(), (uLong)raw.size(), 6) != Z_OK) { err = "zlib compress failed"; return false; }
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) { err = "cannot write " + path; return false; }
    auto be32 = [](uint32_t v, uint8_t *o) { o[0] = (uint8_t)(v >> 24); o[1] = (uint8_t)(v >> 16); o[2] = (uint8_t)(v >> 8); o[3] = (uint8_t)v; };
    auto chunk = [&](const char *tag, const uint8_t *data, uint32_t n) {
        uint8_t hdr[8]; be32(n, hdr); std::memcpy(hdr + 4, tag, 4);
        std::fwrite(hdr, 1, 8, f); if (n) std::fwrite(data, 1, n, f);
        uLong c = crc32(0L, (const Bytef *)tag, 4); if (n) c = crc32(c, data, n);
        uint8_t cb[4]; be32((uint32_t)c, cb); std::fwrite(cb, 1, 4, f);
    };
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    std::fwrite(sig, 1, 8, f);
    uint8_t ihdr[13]; be32((uint32_t)w, ihdr); be32((uint32_t)h, ihdr + 4); ihdr[8] = 8; ihdr[9] = 6; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;
    chunk("IHDR", ihdr, 13); chunk("IDAT", comp.data(), (uint32_t)clen); chunk("IEND", nullptr, 0);
    std::fclose(f);
    return true;
}

// ---- scene dump (for the cross-check against the Python host, tests/test_host_cpp.py) -------------------------
// PTRSDUMP: magic, the PtrsCamera, meshes, materials, textures, lights, then a 12-byte trailer "LENS" + lens_radius + focal_distance
// (readers of the earlier form stop before it).  PTRSDMP2, the full form, has no trailer: its reader holds it to the last byte.
bool dump_scene(const std::string &path, const Camera &cam, const RenderScene &s) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    auto w32 = [&](uint32_t v) { std::fwrite(&v, 4, 1, f); };
    std::fwrite("PTRSDUMP", 1, 8, f);
    std::fwrite(&cam.abi, sizeof(PtrsCamera), 1, f);
    w32((uint32_t)s.meshes.size());
    for (auto &m : s.meshes) {
        w32((uint32_t)(m.pos.size() / 3)); w32((uint32_t)(m.indices.size() / 3)); w32((uint32_t)m.material); w32(m.normal.empty() ? 0u : 1u);
        std::fwrite(m.pos.data(), 4, m.pos.size(), f); std::fwrite(m.normal.data(), 4, m.normal.size(), f); std::fwrite(m.indices.data(), 4, m.indices.size(), f);
    }
    w32((uint32_t)s.materials.size());
    for (auto &m : s.materials) { w32((uint32_t)m.kind); for (int k = 0; k < 6; ++k) w32((uint32_t)m.tex[k]); w32((uint32_t)m.flags); w32((uint32_t)m.inner); }
    w32((uint32_t)s.textures.size());
    for (auto &t : s.textures) { w32((uint32_t)t.kind); w32((uint32_t)t.channels); std::fwrite(t.value, 4, 3, f); std::fwrite(t.value2, 4, 3, f); }
    w32((uint32_t)s.lights.size());
    for (auto &l : s.lights) { w32((uint32_t)l.kind); w32(l.mesh); w32(l.tri); w32((uint32_t)l.ke_tex); }
    std::fwrite("LENS", 1, 4, f); std::fwrite(&cam.lens.lens_radius, 4, 1, f); std::fwrite(&cam.lens.focal_distance, 4, 1, f); // trailer: the thin lens
    std::fclose(f);
    return true;
}

bool dump_scene_full(const std::string &path, const Camera &cam, const RenderScene &s) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    auto w32 = [&](uint32_t v) { std::fwrite(&v, 4, 1, f); };
    auto wf = [&](const float *p, size_t n) { if (n) std::fwrite(p, 4, n, f); };
    std::fwrite("PTRSDMP2", 1, 8, f);
    std::fwrite(&cam.abi, sizeof(PtrsCamera), 1, f);
    w32((uint32_t)s.meshes.size());
    for (auto &m : s.meshes) {
        w32((uint32_t)(m.pos.size() / 3)); w32((uint32_t)(m.indices.size() / 3)); w32((uint32_t)m.material); w32((uint32_t)m.alpha_mask_tex);
        w32((m.normal.empty() ? 0u : 1u) | (m.uv.empty() ? 0u : 2u) | (m.tangent.empty() ? 0u : 4u));
        wf(m.pos.data(), m.pos.size()); wf(m.normal.data(), m.normal.size()); wf(m.uv.data(), m.uv.size()); wf(m.tangent.data(), m.tangent.size());
        std::fwrite(m.indices.data(), 4, m.indices.size(), f);
    }
    w32((uint32_t)s.materials.size());
    for (auto &m : s.materials) { w32((uint32_t)m.kind); for (int k = 0; k < 6; ++k) w32((uint32_t)m.tex[k]); w32((uint32_t)m.flags); w32((uint32_t)m.inner); }
    w32((uint32_t)s.textures.size());
    for (auto &t : s.textures) {
        w32((uint32_t)t.kind); w32((uint32_t)t.channels); wf(t.value, 3); wf(t.value2, 3); wf(&t.su, 1); wf(&t.sv, 1); wf(&t.du, 1); wf(&t.dv, 1);
        w32((uint32_t)t.wrap); w32((uint32_t)t.n_levels);
        for (int l = 0; l < t.n_levels; ++l) { w32((uint32_t)t.level_cols[l]); w32((uint32_t)t.level_rows[l]); wf(t.level_data[l], (size_t)t.level_cols[l] * t.level_rows[l] * t.channels); }
    }
    w32((uint32_t)s.lights.size());
    for (auto &l : s.lights) {
        w32((uint32_t)l.kind); wf(l.v, 3); wf(l.c, 3); w32(l.mesh); w32(l.tri); w32((uint32_t)l.ke_tex); w32((uint32_t)l.lmap_tex);
        wf(l.light_to_world, 16); wf(l.world_to_light, 16); w32((uint32_t)l.dist_nu); w32((uint32_t)l.dist_nv);
        if (l.kind == PTRS_LIGHT_INFINITE) {
            const size_t nu = (size_t)l.dist_nu, nv = (size_t)l.dist_nv;
            wf(l.dist_func, nu * nv); wf(l.dist_cdf, (nu + 1) * nv); wf(l.dist_func_int, nv); wf(l.marg_cdf, nv + 1); wf(&l.marg_func_int, 1);
        }
    }
    std::fclose(f);
    return true;
}

} // namespace ptrs_host
