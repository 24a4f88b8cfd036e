/*
 * ptrs.h -- C ABI of the MI355X wavefront path-tracing backend ("ptrs").
 *
 * Drop-in boundary: the reference has no FFI; its hot path is entered through one Rust method
 *     impl PathIntegrator { pub fn render(&self, camera: &Camera, scene: &RenderScene) }
 *                                                   (src/pathtracer/integrator.rs:536)
 * called from src/headless.rs:216,227, src/viewer/mod.rs:115, benches/benchmark_pathtracer.rs:30.
 * Everything that call reads (immutable scene, camera, sampler/integrator parameters) crosses
 * this ABI as flat plain-old-data; the only thing it writes (the film accumulators,
 * src/common/film.rs:113-129) comes back as 16-byte pixels.  INTEGRATION.md shows the Rust
 * `extern "C"` binding a maintainer would add.
 *
 * Conventions: caller owns every host buffer (they may be freed after ptrs_scene_create /
 * ptrs_render return); the library owns device memory; all entry points return PTRS_OK (0) or a
 * negative error code and never abort; ptrs_last_error() gives the message for the calling
 * thread.  One render at a time per PtrsScene.  All matrices are row-major 4x4.
 */
#ifndef PTRS_H
#define PTRS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTRS_ABI_VERSION 4

enum {
    PTRS_OK = 0,
    PTRS_ERR_INVALID = -1,     /* bad argument / inconsistent description */
    PTRS_ERR_UNSUPPORTED = -2, /* a record kind this build does not implement */
    PTRS_ERR_DEVICE = -3,      /* HIP runtime failure (no GPU, OOM, launch error) */
    PTRS_ERR_IO = -4
};

/* ---- textures (src/pathtracer/texture.rs:15-192,238-465) ---------------------------------- */
enum { PTRS_TEX_CONSTANT = 0, PTRS_TEX_CHECKER = 1, PTRS_TEX_IMAGE = 2 };
enum { PTRS_WRAP_REPEAT = 0, PTRS_WRAP_BLACK = 1, PTRS_WRAP_CLAMP = 2 }; /* common/mod.rs:65-70 */

typedef struct PtrsTexture {
    int32_t kind;     /* PTRS_TEX_* */
    int32_t channels; /* 1 = f32 texture, 3 = Spectrum / Vector3 texture */
    float value[3];   /* CONSTANT: the value.  CHECKER: v1 (texture.rs:56-60) */
    float value2[3];  /* CHECKER: v2 */
    float su, sv, du, dv; /* UVMap (texture.rs:29-53); ignored by CONSTANT */
    int32_t wrap;     /* IMAGE: PTRS_WRAP_* */
    int32_t n_levels; /* IMAGE: MIP pyramid built by the host exactly as MIPMap::new (279-405) */
    const float *const *level_data; /* n_levels pointers; level l is rows*cols*channels f32,
                                        row-major, row index = t, column = s (texel(): 245-273) */
    const int32_t *level_cols;
    const int32_t *level_rows;
} PtrsTexture;

/* ---- materials (src/pathtracer/material/{mod,metal,substrate,disney}.rs) ------------------- */
enum {
    PTRS_MAT_MATTE = 0,     /* tex[0]=kd                                   mod.rs:143-167 */
    PTRS_MAT_METAL = 1,     /* tex[0]=eta [1]=k [2]=r [3]=roughness [4]=u_rough [5]=v_rough
                               (-1 = absent), flags&1 = remap_roughness    metal.rs:49-94 */
    PTRS_MAT_MIRROR = 2,    /*                                             mod.rs:169-195 */
    PTRS_MAT_GLASS = 3,     /* tex[0]=kr [1]=kt [2]=index                  mod.rs:197-256 */
    PTRS_MAT_DISNEY = 4,    /* tex[0]=color [1]=metallic [2]=eta [3]=roughness  disney.rs:172-264 */
    PTRS_MAT_SUBSTRATE = 5, /* tex[0]=kd [1]=ks [2]=nu [3]=nv, flags&1 = remap  substrate.rs:42-68 */
    PTRS_MAT_NORMAL = 6     /* tex[0]=normal map (3-channel), inner = wrapped material  mod.rs:39-79,125-141 */
};

typedef struct PtrsMaterial {
    int32_t kind;
    int32_t tex[6];
    int32_t flags;
    int32_t inner;
} PtrsMaterial;

/* ---- geometry (src/pathtracer/shape.rs:581-641, primitive.rs:20-24) ------------------------ */
typedef struct PtrsMesh {
    uint32_t n_verts;
    uint32_t n_tris;
    const float *pos;        /* n_verts*3, WORLD space (TriangleMesh::new_with_transform 592-623) */
    const float *normal;     /* n_verts*3 or NULL */
    const float *tangent;    /* n_verts*3 or NULL ("s") */
    const float *uv;         /* n_verts*2 or NULL -> default (0,0),(1,0),(1,1) (shape.rs:34-48) */
    const uint32_t *indices; /* n_tris*3 */
    int32_t material;        /* index into materials[] (one GeometricPrimitive per triangle) */
    int32_t alpha_mask_tex;  /* 1-channel texture or -1 (shape.rs:228-244,471-521) */
    int32_t reverse_orientation;        /* always 0 in the reference (shape.rs:626-641) */
    int32_t transform_swaps_handedness; /* always 0 in the reference */
} PtrsMesh;

/* ---- lights (src/pathtracer/light.rs) ------------------------------------------------------ */
enum { PTRS_LIGHT_POINT = 0, PTRS_LIGHT_DIRECTIONAL = 1, PTRS_LIGHT_AREA = 2, PTRS_LIGHT_INFINITE = 3 };

typedef struct PtrsLight {
    int32_t kind;
    float v[3]; /* POINT: p_light (86-97).  DIRECTIONAL: w_light, already normalised (159-171) */
    float c[3]; /* POINT: I.  DIRECTIONAL: L */
    /* AREA: one DiffuseAreaLight per emissive triangle (231-250; mitsuba.rs:309-323) */
    uint32_t mesh, tri;
    int32_t ke_tex; /* 3-channel emission texture */
    /* DIRECTIONAL / INFINITE: Light::preprocess (209-211, 480-482; bounds.rs:126-134) */
    float world_center[3];
    float world_radius;
    /* INFINITE (321-503) */
    int32_t lmap_tex; /* 3-channel IMAGE texture (the MIPMap), wrap = REPEAT */
    float light_to_world[16];
    float world_to_light[16];
    int32_t dist_nu, dist_nv;   /* Distribution2D dimensions (sampling.rs:185-230) */
    const float *dist_func;     /* nv*nu      conditional func */
    const float *dist_cdf;      /* nv*(nu+1)  conditional cdf */
    const float *dist_func_int; /* nv         conditional integrals (= marginal func) */
    const float *marg_cdf;      /* nv+1 */
    float marg_func_int;
} PtrsLight;

/* Optional pre-built accelerator in the reference's flattened layout (accelerator.rs:89-95).
 * When nodes == NULL the library builds its own BVH (closest-hit results do not depend on the
 * tree: SURVEY.md Q29). */
typedef struct PtrsBvhNode {
    float p_min[3];
    float p_max[3];
    uint32_t offset;    /* leaf: first primitive in prim order; interior: second child */
    uint16_t num_prims; /* 0 = interior */
    uint8_t axis;
    uint8_t pad;
} PtrsBvhNode;

typedef struct PtrsSceneDesc {
    uint32_t n_meshes;
    const PtrsMesh *meshes;
    uint32_t n_materials;
    const PtrsMaterial *materials;
    uint32_t n_textures;
    const PtrsTexture *textures;
    uint32_t n_lights;
    const PtrsLight *lights; /* order = RenderScene::lights (sampled uniformly, integrator.rs:204) */
    uint32_t n_bvh_nodes;    /* optional */
    const PtrsBvhNode *bvh_nodes;
    const uint32_t *bvh_prims; /* n_prims entries: global triangle id (mesh-major) in leaf order */
} PtrsSceneDesc;

/* ---- camera (src/common/mod.rs:20-62; pathtracer/mod.rs:59-81) ----------------------------- */
typedef struct PtrsCamera {
    float rot[4];   /* cam_to_world rotation, unit quaternion (i, j, k, w) = nalgebra Isometry3 */
    float trans[3]; /* cam_to_world translation */
    float m00, m11, m22, m23;   /* Perspective3 matrix entries used by unproject_point */
    float raster_to_screen[16]; /* Affine3 */
    float dx_camera[3];
    float dy_camera[3];
} PtrsCamera;

/* Thin-lens camera (no counterpart in the reference, whose CameraSample holds p_film alone, sampler/mod.rs:162-166; DESIGN.md
 * section 15): a PtrsCamera followed by the lens.  With PTRS_FLAG_THIN_LENS in params->flags every entry point that takes
 * (camera, params) reads its `camera` argument as a PtrsCameraLens.  The lens is per call: no scene state, no option.
 * A negative or non-finite lens_radius, or with lens_radius > 0 a focal_distance that is not finite and > 0, is refused
 * (PTRS_ERR_INVALID) before the first device call.  lens_radius == 0 is the pinhole render bit for bit: no lens sample is drawn. */
typedef struct PtrsCameraLens {
    PtrsCamera camera;
    float lens_radius;    /* >= 0, finite; 0 = pinhole */
    float focal_distance; /* distance of the plane in focus from the lens plane along the view axis; finite, > 0 when lens_radius > 0 */
} PtrsCameraLens;

/* ---- render parameters (sampler/sobol.rs:35-60; integrator.rs:219-246) --------------------- */
typedef struct PtrsRenderParams {
    int32_t width, height; /* film resolution (film.rs:132) */
    int32_t spp;           /* rounded up to a power of two like the reference (sobol.rs:37) */
    int32_t max_depth;
    float rr_threshold;     /* reference: 1.0 */
    int32_t rr_start_depth; /* reference: 3 */
    int32_t rr_enable;      /* reference: 1 */
    int32_t row_begin, row_end; /* output rows written by this call; 0,height = whole film.
                                   Multi-GPU ranks each take a band */
    int32_t device;             /* HIP device ordinal */
    uint32_t paths_per_pass;    /* 0 = auto */
    uint32_t flags;             /* PTRS_FLAG_* */
    int32_t sampler;            /* PTRS_SAMPLER_*: the reference builds a SobolSamplerBuilder (main.rs:103); its StratifiedSampler
                                   (sampler/stratified.rs) is compiled but never instantiated (sampler/mod.rs:169-170) */
    int32_t n_sampled_dimensions; /* STRATIFIED: StratifiedSamplerBuilder::new's n_sampled_dimensions; spp = dim_pixel_samples^2.
                                   Must cover the path: >= 3 * (max_depth + 1) + 1, because a draw past it would come straight
                                   from the tile's generator in path order (mod.rs:137-151), which a wavefront cannot reproduce:
                                   such a render is refused (PTRS_ERR_UNSUPPORTED) */
} PtrsRenderParams;
enum { PTRS_SAMPLER_SOBOL = 0, PTRS_SAMPLER_STRATIFIED = 1 };

enum {
    PTRS_FLAG_COUNTERS = 1u, /* fill nodes_visited / tris_tested (slower: device atomics) */
    PTRS_FLAG_TIMING = 2u,   /* hipEvent timing of every kernel launch (needs stream syncs) */
    PTRS_FLAG_FILM_ZERO = 4u, /* ptrs_render_multi: film_inout is all zeros (Film::clear), the devices clear their bands instead of uploading them */
    PTRS_FLAG_THIN_LENS = 8u  /* `camera` points to a PtrsCameraLens.  Sobol': the lens sample is the get_2d behind the film sample (dimensions 2, 3) and the
                                 path's dimension counter starts two higher; stratified: it is the pixel table's second 2-D dimension and the
                                 n_sampled_dimensions requirement rises by one */
};

/* film pixel: linear RGB sums and filter-weight sum (film.rs:113-119; splat_xyz is never
 * written by the reference and is not carried).  Row-major, y*width + x (film.rs:187-191). */
typedef struct PtrsFilmPixel {
    float rgb[3];
    float weight;
} PtrsFilmPixel;

typedef struct PtrsStats {
    uint64_t samples;        /* li() evaluations = (W+4)(H_band+4)*spp */
    uint64_t rays_extension; /* BVH closest-hit queries, integrator.rs:416 */
    uint64_t rays_shadow;    /* BVH any-hit queries, light.rs:40 */
    uint64_t rays_mis;       /* BVH closest-hit queries, integrator.rs:119 */
    uint64_t nodes_visited;  /* only with PTRS_FLAG_COUNTERS */
    uint64_t tris_tested;    /* only with PTRS_FLAG_COUNTERS */
    uint64_t passes;
    uint64_t kernel_launches;
    uint64_t trace_launches;
    double ms_total;    /* wall clock of the call (host timer around the stream) */
    double ms_trace;    /* sum of trace-kernel durations (PTRS_FLAG_TIMING) */
    double ms_shade;    /* generate + sort + shade + resolve kernels (PTRS_FLAG_TIMING) */
    double ms_film;     /* film kernels (PTRS_FLAG_TIMING) */
    uint64_t bvh_nodes;
    uint64_t bvh_max_depth;
    uint64_t device_bytes; /* peak device allocation of the call */
    /* PTRS_FLAG_TIMING, per kernel class: durations summed over the launches of the call, and the launch counts.
     * ms_trace = ms_extend + ms_connect; ms_shade = ms_shade_kernels + ms_aux. */
    double ms_extend;        /* extension-ray traversal kernels (k_extend / k_extend_rf) */
    double ms_connect;       /* shadow + MIS ray traversal kernels (k_connect / k_connect_rf) */
    double ms_shade_kernels; /* k_shade<material, features> */
    double ms_aux;           /* k_generate, k_epilogue, k_resolve */
    uint64_t extend_launches, connect_launches, shade_launches, aux_launches, film_launches;
    uint64_t error_flags;    /* PTRS_ERRFLAG_* raised by device code (render returns PTRS_ERR_UNSUPPORTED) */
    /* PTRS_FLAG_COUNTERS, lane-refill traversal kernels: lane occupancy of the two phases =
     * node_visits / node_steps_x64 and tris_tested (of these kernels) / tri_steps_x64 */
    uint64_t node_steps_x64, node_visits, tri_steps_x64;
    uint64_t debug[12];      /* zero in product builds; diagnostic builds (-DPTRS_STAMPS): wave-clock sums per phase of k_shade; ptrs_denoise with PTRS_DENOISE_TIMING: nanoseconds per launch */
    /* how the queue kernels of the call's last pass were launched (ABI 3): segments per queue (one wave each), and per kernel class
     * [0] extend, [1] connect, [2] shade, [3] aux the workgroups of the last launch and the resident workgroups per CU the launch was
     * sized for (hipOccupancyMaxActiveBlocksPerMultiprocessor, capped by what the CU's LDS holds in allocation granules) */
    uint64_t queue_segments;
    uint64_t grid_wgs[4];
    uint64_t resident_wgs_per_cu[4];
    uint64_t lanes;          /* pipeline lanes the call ran on (option "lanes", or chosen by the size of the job) */
    uint64_t grid_pct;       /* share of a kernel's resident capacity its launches took (option "grid_pct", or chosen with the lanes) */
    double ms_enqueue;       /* host time from the start of the call until its last pass was enqueued (a job of more passes than lanes
                              * waits for a lane in between); ms_total - ms_enqueue is what the host then waited for the device */
    /* ABI 4: the fused tail (one launch per pass in which every wave takes its queue segment through all remaining rounds) */
    double ms_tail;          /* its kernels (PTRS_FLAG_TIMING; their traversal and shading are not in ms_trace / ms_shade) */
    uint64_t tail_launches;
    uint64_t tail_round;     /* the round at which the call's last pass handed over, 0xffffffff: it did not */
    /* the traversal form the scene's kernels were chosen for: LDS stack entries per lane (8, 9 or 16), and the 16-byte vectors the
     * scene's pair tree and triangles take in LDS form (0: quad form, traversed out of memory) */
    uint64_t stack_lds;
    uint64_t lds_form_v4;
} PtrsStats;

enum {
    PTRS_ERRFLAG_SOBOL_DIM = 1u,  /* a path needed Sobol dimension >= 1024 (the reference panics: sobol.rs:177-183) */
    PTRS_ERRFLAG_NULL_SKIPS = 2u  /* paths still alive after max_depth + 1 + 64 rounds of null-BSDF skips */
};

typedef struct PtrsScene PtrsScene;

/* Process-wide tuning knobs; the library reads no environment variables.  Names: "lanes" (1-8 concurrent pipeline lanes;
 * 0 = four, one for a job under 4 M paths), "grid_mult" (queue segments -- one wave each -- per pass = CUs x 8 x grid_mult; 0 = 1
 * with several lanes -- up to 4 for scenes whose tree is traversed out of HBM / L2, by the paths of a pass --, 8 with one), "grid_pct" (share of its resident capacity a persistent launch takes; 0 = 100, or 50 with several
 * lanes and a grid_mult given by hand), "persist" (0/1), "whole_rounds" (0/1), "refill" / "refill_connect" (idle-lane threshold of the
 * lane-refill traversal kernels, 0 = refill only when the whole wave is idle, -1 = by scene), "vote" (phase voting in the traversal
 * kernels: 0 off, 1 on, 2 extension kernel only, -1 = by scene), "stack_lds" (8 or 16 LDS stack entries per lane), "shade_lds"
 * (0/1: shade kernels read their small tables from LDS), "env_presample" (0/1: environment-light samples evaluated ahead of the
 * shade kernels), "fused_epilogue" / "fused_resolve" (0/1: the traversal kernels run the segment's epilogue / MIS resolve behind
 * the wave's last ray instead of separate k_epilogue / k_resolve launches), "node_form" (0 auto, 2 force quad nodes), "node_order"
 * (0 / 1: quad-node order behind the LDS-cached top), "workspace_pct" (share of the free device memory the render workspace may
 * take, default 40), "peer_copy" (0: ptrs_render_multi stages bands through the host film).  None of them changes a result bit;
 * they select between equivalent schedules.  Scene-level knobs (node_form, node_order, stack_lds) are read by
 * ptrs_scene_create, the rest by each render call.  Replaces nothing in the reference (its only knobs are the CLI flags of
 * main.rs:36-52). */
int ptrs_set_option(const char *name, int64_t value);
int ptrs_get_option(const char *name, int64_t *value);
/* The same knobs for ONE scene: its renders take this value instead of the process-wide one (two embedders in a process, or
 * two scenes of one embedder, can differ).  Knobs read at scene creation (node_form, stack_lds) are not affected. */
int ptrs_scene_set_option(PtrsScene *scene, const char *name, int64_t value);

int ptrs_abi_version(void);
/* Identity of this build: a hash over the kernel sources and every compiler flag (pathtracer-rs_amd/build.py).  Measurement files
 * under profiles/ record it; bench.py takes hardware counters only from a file measured with the library it runs. */
const char *ptrs_build_id(void);
int ptrs_abi_sizeof(int which); /* sizeof the ABI structs as compiled (binding self-check) */
const char *ptrs_last_error(void);

/* Uploads the scene and (unless desc->bvh_nodes is given) builds the accelerator on the host.
 * Replaces: RenderScene construction hand-off, the precedent being OptixAccelerator::new(&scene)
 * (src/pathtracer/gpu/optix.rs:160-290) which consumes the same flat mesh arrays.
 *
 * The description is checked, and the host copy built, BEFORE the first device call: a description that breaks a rule below is refused
 * with PTRS_ERR_INVALID (an unknown material or light kind: PTRS_ERR_UNSUPPORTED) and a message that names the rule, on a machine
 * without a GPU too; a valid one gets PTRS_ERR_DEVICE there.  Nothing of a refused description reaches a device.
 *  - A non-zero count comes with its array: meshes, materials, textures, lights; an IMAGE texture's level_data, level_cols, level_rows
 *    and every level_data[l]; an INFINITE light's four tables; bvh_prims with bvh_nodes.
 *  - Textures: kind 0..2, channels 1 or 3; IMAGE: n_levels >= 1, every level at least 1 x 1, wrap one of PTRS_WRAP_*.
 *  - Materials: every tex[k] is -1 or a texture; the slots the kind names hold textures of the channel counts above (Metal: `roughness`,
 *    or u_rough and v_rough together, all 1-channel); NORMAL: inner is another material, and a chain of wrappers reaches a material of
 *    another kind within four steps (no wrapper of itself, no cycle), whether a mesh uses it or not.
 *  - Meshes: material in range, alpha_mask_tex -1 or a 1-channel texture.  A mesh with n_tris == 0 is legal whatever its pointers and its
 *    vertex count are: none is read, and it contributes nothing (later meshes keep their global triangle ids).  With triangles: pos and
 *    indices present, every index < n_verts, every position finite -- a NaN or an infinity is refused, the message names mesh and vertex.
 *  - A scene without any triangle (no mesh, or only empty ones) is legal: every ray misses, the lights that need no geometry still
 *    shine.  ptrs_scene_info and PtrsStats::bvh_nodes then report the one traversal record no ray can enter: 1 node, 0 triangles.
 *  - Lights: AREA names a triangle of a mesh and a 3-channel ke_tex; INFINITE a 3-channel IMAGE lmap_tex and dist_nu, dist_nv >= 1.
 *  - A pre-built tree: a leaf's range [offset, offset + num_prims) lies within the triangles (tested in 64 bits); an interior node's
 *    offset is a node, its first child i + 1 exists, its axis is 0..2; every bvh_prims entry is a triangle id; and walking from node 0,
 *    every node is reached EXACTLY once (no node shared by two parents, none skipped, no cycle) at a depth of at most 4096.  The check
 *    is linear in the description's size. */
int ptrs_scene_create(const PtrsSceneDesc *desc, int32_t device, PtrsScene **out);
void ptrs_scene_destroy(PtrsScene *scene);
/* accelerator facts (the reference logs these: accelerator.rs:131-148); any pointer may be NULL */
int ptrs_scene_info(PtrsScene *scene, uint64_t *n_nodes, uint64_t *max_depth, uint64_t *n_tris);

/* PathIntegrator::render (integrator.rs:536-642).  ACCUMULATES into film_inout (host memory,
 * width*height pixels) like Film::merge_film_tile (film.rs:213-228); rows outside
 * [row_begin,row_end) are untouched.  stats may be NULL. */
int ptrs_render(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params,
                PtrsFilmPixel *film_inout, PtrsStats *stats);

/* render with the film visible while it forms -- what the reference's preview thread gets by reading the shared film
 * every two seconds while render() runs (headless.rs:197-214).  After every pass of the
 * wavefront pipeline (a block of sample rows x a block of sample indices) whose film kernel has finished, the output rows
 * it touched are copied into film_inout and `fn(user, passes_done, passes_total, row_begin, row_end)` is called on the
 * calling thread; the rows hold the samples accumulated so far (rgb and weight sums: divide to display, film.rs:253-271):
 * at least those of the passes reported so far -- the copy is taken when the pass's pipeline lane is next waited for, passes
 * behind it keep running and may already show -- and callbacks arrive in pass order.
 * The final film is bit-identical to ptrs_render's. */
typedef void (*PtrsProgressFn)(void *user, uint32_t passes_done, uint32_t passes_total, int32_t row_begin, int32_t row_end);
int ptrs_render_progressive(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params,
                            PtrsFilmPixel *film_inout, PtrsProgressFn fn, void *user, PtrsStats *stats);

/* One process, several devices (the reference host is one process: main.rs:101-126).  scenes[i] is the same scene
 * created on device i (ptrs_scene_create with that ordinal); output rows [band_bounds[i], band_bounds[i+1]) are rendered
 * by scenes[i] on a host thread of its own, gathered into scenes[0]'s device with peer copies and returned in
 * film_inout (host, ACCUMULATED like ptrs_render).  band_bounds: n+1 row numbers from 0 to height, or NULL for equal
 * bands; ptrs_plan_bands computes them, optionally weighted by a per-row cost (row_cost[height], e.g. ray counts of
 * a 1-spp probe; NULL = equal rows).  stats_per_scene: n records or NULL.  Bit-identical to ptrs_render. */
int ptrs_plan_bands(int32_t height, uint32_t n, const float *row_cost, int32_t *bounds_out /* n + 1 */);
/* The per-row cost for ptrs_plan_bands, measured: `params`' render (give spp = 1) with one device counter per sample row -- every BVH
 * query a path makes is added to its row -- and no film; row_cost_out[height] = queries of the sample row under each output row.  One
 * call of a few milliseconds; what it replaces is the reference's dynamic tile queue (integrator.rs:617-637), which balances at run
 * time what a static band split has to know beforehand. */
int ptrs_render_row_cost(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, float *row_cost_out, PtrsStats *stats);
int ptrs_render_multi(PtrsScene *const *scenes, uint32_t n, const PtrsCamera *camera,
                      const PtrsRenderParams *params, const int32_t *band_bounds,
                      PtrsFilmPixel *film_inout, PtrsStats *stats_per_scene);

/* Same, but the film lives in DEVICE memory (width*height PtrsFilmPixel) and the work is queued
 * on `hip_stream` (a hipStream_t, NULL = default stream); returns after the stream has drained.
 * This is what bench.py times and what the multi-GPU gather reads. */
int ptrs_render_device(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params,
                       void *film_inout_device, void *hip_stream, PtrsStats *stats);

/* Test/debug form of render: additionally returns the radiance of every sample,
 * sample_rgb[((sy*(W+4) + sx)*spp + s)*3 + c] for sample-pixel (sx,sy) relative to the sample
 * bounds' p_min (film.rs:174-185), i.e. the value `l` at integrator.rs:579.  Host memory. */
int ptrs_render_samples(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params,
                        PtrsFilmPixel *film_inout, float *sample_rgb, PtrsStats *stats);

/* First-hit feature planes for a denoiser or a compositor (no counterpart in the reference): albedo, shading normal and depth +
 * coverage of the camera samples of `params`' render, filtered onto the film by exactly the samples and weights of the beauty image
 * (same sampler, sample grid, row bands and pass plan; max_depth is ignored: the pass ends behind its first extension, and a specular
 * first hit is not followed).  planes: which planes to gather (plane k = bit k); planes_inout[k]: that plane's film, ACCUMULATED like
 * ptrs_render's -- rgb = sums of albedo | shading normal | (depth, coverage, 0) times the filter weight, weight = the filter-weight sum.
 * Albedo is the base colour slot of the innermost material (Matte kd, Metal r, Glass kr, Disney color, Substrate kd; Mirror and an
 * absent slot: 1, 1, 1); a sample that misses contributes zeros.  sample_aov: NULL, or 12 floats per sample laid out like
 * ptrs_render_samples' sample_rgb: albedo.rgb, coverage, normal.xyz, depth, position.xyz, the triangle id's bit pattern (0xffffffff:
 * miss); samples outside the call's sample rows stay 0.  The _device form takes the planes (and sample_aov) in device memory and a stream. */
enum { PTRS_AOV_ALBEDO = 1u, PTRS_AOV_NORMAL = 2u, PTRS_AOV_DEPTH = 4u };
#define PTRS_AOV_PLANES 3
#define PTRS_AOV_SAMPLE_FLOATS 12
int ptrs_render_aov(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, uint32_t planes,
                    PtrsFilmPixel *const planes_inout[PTRS_AOV_PLANES], float *sample_aov, PtrsStats *stats);
int ptrs_render_aov_device(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, uint32_t planes,
                           void *const planes_inout_device[PTRS_AOV_PLANES], float *sample_aov_device, void *hip_stream, PtrsStats *stats);

/* Edge-avoiding a-trous denoiser of a low-spp film, guided by the three planes of ptrs_render_aov (no counterpart in the reference;
 * the contract is DESIGN.md section 11).  Inputs: four accumulated films of width x height pixels -- beauty (ptrs_render) and the
 * albedo, normal and depth planes, all three required; they are never written.  out (width x height, not one of the inputs) receives
 * rgb = the filtered colour, weight = 1; a pixel without weight gives zeros.  iterations: 1 .. PTRS_DENOISE_MAX_ITERATIONS, iteration i
 * has taps 2^i pixels apart and colour sigma sigma_color / 2^i; a sigma <= 0 drops its term.  PTRS_DENOISE_DEMODULATE: the colour is
 * divided by the albedo before the filter and multiplied by it afterwards.  A PtrsDenoiser owns the workspace (64 bytes per pixel) of
 * one device for one width x height; one call at a time per denoiser.  It never touches a PtrsScene.  The argument checks are made
 * before the first device call.  stats (may be NULL): ms_total, kernel_launches and device_bytes, everything else 0 (PTRS_DENOISE_TIMING apart).  The _device form
 * takes the films in device memory and a stream, and returns after the stream has drained.  Option "denoise_lds" (-1 = by step, 0, 1)
 * selects between two forms of the iteration kernel (direct loads / an LDS-staged tile, steps up to 16); it changes no bit. */
#define PTRS_DENOISE_MAX_ITERATIONS 8
enum {
    PTRS_DENOISE_DEMODULATE = 1u,
    PTRS_DENOISE_TIMING = 2u /* measurement hook (tools/denoise_cost.py): hipEvent time of every launch of the call, in nanoseconds, in
                                stats->debug: [0] prepare, [1 + i] iteration i, [9] finish.  Changes no bit of the output */
};
typedef struct PtrsDenoiseParams {
    int32_t iterations;
    float sigma_color, sigma_normal, sigma_depth;
    uint32_t flags; /* PTRS_DENOISE_* */
} PtrsDenoiseParams;
typedef struct PtrsDenoiser PtrsDenoiser;
void ptrs_denoise_default_params(PtrsDenoiseParams *p); /* 5 iterations, sigmas 0.25 / 0.3 / 0.1, demodulation on */
int ptrs_denoiser_create(int32_t device, int32_t width, int32_t height, PtrsDenoiser **out);
void ptrs_denoiser_destroy(PtrsDenoiser *d);
int ptrs_denoise(PtrsDenoiser *d, const PtrsDenoiseParams *p, const PtrsFilmPixel *beauty,
                 const PtrsFilmPixel *const planes[PTRS_AOV_PLANES], PtrsFilmPixel *out, PtrsStats *stats); /* host memory */
int ptrs_denoise_device(PtrsDenoiser *d, const PtrsDenoiseParams *p, const void *beauty_device,
                        const void *const planes_device[PTRS_AOV_PLANES], void *out_device, void *hip_stream, PtrsStats *stats);

/* Sample ranges, the film's error and rendering until it has converged (no counterpart in the reference, which renders a fixed spp;
 * the contracts are DESIGN.md section 12).
 *
 * ptrs_render_range: samples [sample_begin, sample_end) of `params`' render -- params->spp stays the WHOLE render's count (rounded up
 * to a power of two as always; the stratified sampler takes it as is) -- accumulated into film_inout like ptrs_render, and, when
 * film_half_inout is given (it must not be film_inout), into that film as well by a second gather of the same passes.  Refused with
 * PTRS_ERR_INVALID before any device call unless sample_begin < sample_end <= the rounded spp.  row_begin / row_end as in ptrs_render.
 * sample_rgb (may be NULL) has ptrs_render_samples' layout with the absolute sample number; only the range's entries are written.
 * stats are those of the range.  With a pass plan that keeps the band's rows in one pass, successive ranges that tile [0, spp) give
 * ptrs_render's film bit for bit.  The _device form takes the films in device memory and a stream. */
int ptrs_render_range(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, uint32_t sample_begin, uint32_t sample_end,
                      PtrsFilmPixel *film_inout, PtrsFilmPixel *film_half_inout, float *sample_rgb, PtrsStats *stats);
int ptrs_render_range_device(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, uint32_t sample_begin, uint32_t sample_end,
                             void *film_inout_device, void *film_half_inout_device, void *hip_stream, PtrsStats *stats);

/* ptrs_film_error: how far a film is from the film of half of its samples (the half-buffer measure of Dammertz et al.'s stopping
 * condition), per 16 x 16 tile (clipped at the right and bottom edges; tile index = ty * tiles_x + tx) and for the whole film.
 * Per pixel, in binary32: valid = both weights > 0; I = film.rgb / film.weight, A = half.rgb / half.weight,
 * e = ((|I.r - A.r| + |I.g - A.g|) + |I.b - A.b|) / sqrt(max((I.r + I.g) + I.b, 1e-3)), a NaN or infinite e becomes +inf; an invalid
 * pixel has e = 0 and is not counted.  Per tile: error = the sum of e (stride-halving tree over the tile's 256 slots) / valid, 0 for a
 * tile without a valid pixel.  Summary: the largest tile error, the lowest tile index that has it, the valid pixels of the film.
 * The films are never written; film and half must differ.  The argument checks are made before the first device call.  The _device
 * form takes device pointers (tiles_out_device is required: tiles_x * tiles_y records) and a stream; summary_out is host memory. */
typedef struct PtrsTileError { float error; uint32_t valid; } PtrsTileError;
typedef struct PtrsFilmErrorSummary {
    float max_tile_error;
    uint32_t worst_tile;
    uint64_t valid_pixels;
    uint32_t tiles_x, tiles_y;
} PtrsFilmErrorSummary;
#define PTRS_ERROR_TILE 16
int ptrs_film_error(int32_t device, int32_t width, int32_t height, const PtrsFilmPixel *film, const PtrsFilmPixel *half,
                    PtrsTileError *tiles_out /* may be NULL */, PtrsFilmErrorSummary *summary_out);
int ptrs_film_error_device(int32_t device, int32_t width, int32_t height, const void *film_device, const void *half_device,
                           void *tiles_out_device, void *hip_stream, PtrsFilmErrorSummary *summary_out);

/* Render until converged.  params->spp is the ceiling, min_spp a power of two in 2 .. spp, target_error finite and >= 0.  The schedule
 * (ptrs_converge_schedule, a pure function): block 0 is [0, min_spp), block k is [n, 2n) with n the samples before it; the first half
 * of every block goes to the film and the half film, the second half to the film only, so the half film always holds n / 2 of the n
 * samples; behind every block ptrs_film_error is asked, and the render stops when max_tile_error < target_error or n = spp.  The two
 * films stay on the device, only the summary crosses to the host per check.  film_inout (host) ACCUMULATES like ptrs_render (the
 * measure means what it says for a film that starts cleared); film_half_out (may be NULL) receives the half film.  history_out: one
 * record per check, at most PTRS_CONVERGE_MAX_CHECKS.  stats (may be NULL): samples, rays, passes and launches summed over the blocks.
 * The film after stopping at n is the film of ptrs_render_range(0, n); at n = spp it is ptrs_render's, bit for bit. */
#define PTRS_CONVERGE_MAX_CHECKS 32
typedef struct PtrsConvergeCheck { uint32_t spp; float max_tile_error; } PtrsConvergeCheck;
typedef struct PtrsConvergeResult {
    uint32_t spp_done;
    uint32_t converged; /* 1: the last check was below the target */
    uint32_t n_checks;
    uint32_t worst_tile; /* of the last check */
    PtrsConvergeCheck history[PTRS_CONVERGE_MAX_CHECKS];
} PtrsConvergeResult;
/* blocks_out: 3 numbers per block -- begin, middle, end: [begin, middle) goes to both films, [middle, end) to the film only; at most
 * PTRS_CONVERGE_MAX_CHECKS blocks.  Refuses (PTRS_ERR_INVALID) an spp or min_spp that is no power of two, or min_spp outside 2 .. spp. */
int ptrs_converge_schedule(uint32_t spp, uint32_t min_spp, uint32_t *blocks_out, uint32_t *n_blocks_out);
int ptrs_render_converged(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, float target_error, uint32_t min_spp,
                          PtrsFilmPixel *film_inout, PtrsFilmPixel *film_half_out, PtrsConvergeResult *result_out, PtrsStats *stats);

/* Adaptive sampling: a sample range on SOME of the film's tiles, and a render that stops tile by tile (no counterpart in the reference;
 * DESIGN.md section 13).  The tiles are those of ptrs_film_error: PTRS_ERROR_TILE x PTRS_ERROR_TILE pixels, origin (0, 0), clipped at
 * the right and bottom edges, index ty * tiles_x + tx.
 *
 * ptrs_render_tiles is ptrs_render_range restricted to the active tiles.  tile_active: tiles_x * tiles_y bytes in HOST memory (both
 * forms), non-zero = active.
 *  - A sample pixel with raster pixel (px, py) is active iff a pixel of [px - 2, px + 2] x [py - 2, py + 2] lies in an active tile (the
 *    active tiles dilated by the filter radius: a sample at p in [px, px + 1) reaches exactly the pixels px - 2 .. px + 2).  Exactly
 *    the samples [sample_begin, sample_end) of the active sample pixels are traced, each once -- adjacent active tiles share their
 *    apron.  stats->samples = active sample pixels x (sample_end - sample_begin); the ray counts are those of these paths.
 *  - Every pixel of an active tile ends with the bits ptrs_render_range leaves there with the same arguments and the same starting
 *    film -- rgb and weight, film and half film; every pixel of an inactive tile keeps its bits.  (ptrs_render_range's own caveat: a
 *    pass plan that splits the rows is held to 1e-6, not to bits; sample chunks change no bit.)
 *  - sample_rgb (may be NULL): the range's entries of the active sample pixels are written and equal ptrs_render_samples'; every other
 *    entry keeps what the caller put there.
 *  - All tiles active: ptrs_render_range bit for bit, statistics included except passes and launches.  No tile active: PTRS_OK, no
 *    device launch, the films untouched, zeroed stats.
 *  - Refused (PTRS_ERR_INVALID) before the first device call: null arguments, a bad sample range, the half film being the film, a row
 *    band in params (the tile form renders the whole film).
 *
 * ptrs_render_adaptive: ptrs_render_converged's schedule (ptrs_converge_schedule), every block on the tiles still active.  All tiles
 * are active for block 0; behind every block ptrs_film_error is asked, and a tile that took part in the block and whose error is
 * < target_error is frozen: never active again, so its pixels and its error stay.  (target_error = 0 freezes nothing.)  The render
 * stops when no tile is active (converged: every tile's error is below the target) or n = spp.  Arguments are checked like
 * ptrs_render_converged's, with its messages.  tile_spp_out (may be NULL, tiles_x * tiles_y entries): the samples tile t's pixels hold.
 * Per check the result carries the samples, the tiles that took part in the block and the largest tile error over ALL tiles.
 * Tile t of the final film is, bit for bit, tile t of ptrs_render_range(0, tile_spp[t]) on the same starting film; while a tile is
 * active its error at every check equals its error in the ptrs_render_converged run, so tile_spp[t] is the first schedule point at
 * which that run's error of tile t is below the target, or spp.  The films stay on the device between the blocks; per check the
 * summary and the tile records (8 bytes per tile) cross to the host. */
typedef struct PtrsAdaptiveCheck { uint32_t spp; uint32_t tiles_active; float max_tile_error; } PtrsAdaptiveCheck;
typedef struct PtrsAdaptiveResult {
    uint32_t spp_done;   /* the samples of the tiles that were active to the end */
    uint32_t converged;  /* 1: no tile is active */
    uint32_t n_checks;
    uint32_t worst_tile; /* of the last check */
    uint32_t tiles_x, tiles_y;
    PtrsAdaptiveCheck history[PTRS_CONVERGE_MAX_CHECKS];
} PtrsAdaptiveResult;
int ptrs_render_tiles(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, uint32_t sample_begin, uint32_t sample_end,
                      const uint8_t *tile_active, PtrsFilmPixel *film_inout, PtrsFilmPixel *film_half_inout, float *sample_rgb, PtrsStats *stats);
int ptrs_render_tiles_device(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, uint32_t sample_begin, uint32_t sample_end,
                             const uint8_t *tile_active, void *film_inout_device, void *film_half_inout_device, void *hip_stream, PtrsStats *stats);
int ptrs_render_adaptive(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, float target_error, uint32_t min_spp,
                         PtrsFilmPixel *film_inout, PtrsFilmPixel *film_half_out, uint32_t *tile_spp_out, PtrsAdaptiveResult *result_out, PtrsStats *stats);
/* The freeze rule (a pure function, no device): next_out[t] = 1 where active[t] is non-zero and tiles[t].error is not < target_error,
 * else 0 (next_out may be active); *n_active_out = how many stay active. */
int ptrs_adaptive_freeze(const PtrsTileError *tiles, uint32_t n_tiles, float target_error, const uint8_t *active, uint8_t *next_out, uint32_t *n_active_out);

/* Feature planes for sample ranges and tiles, and the planes of an adaptive film (no counterpart in the reference; DESIGN.md section
 * 14).  planes / planes_inout / sample_aov as in ptrs_render_aov; every _device form takes the planes (and sample_aov) in device memory
 * and a stream; tile_active and tile_spp are HOST memory in both forms.
 *
 * ptrs_render_aov_range: samples [sample_begin, sample_end) of `params`' AOV call, accumulated into the planes.  params->spp stays the
 * whole render's count (the differential scale 1 / sqrt(spp) is the whole render's).  sample_aov has ptrs_render_aov's layout with the
 * absolute sample number; only the range's entries are written.  Ranges that tile [0, spp) in order, from the same starting planes, give
 * ptrs_render_aov's planes and samples bit for bit under every pass plan.  Refused (PTRS_ERR_INVALID) before the first device call, with
 * ptrs_render_range's messages, unless sample_begin < sample_end <= the rounded spp.
 *
 * ptrs_render_aov_tiles: the range form restricted to the active tiles under ptrs_render_tiles' rules -- the same dilation rule;
 * exactly the range's samples of the active sample pixels are traced, each once; every pixel of an active tile ends with the bits
 * ptrs_render_aov_range leaves there from the same starting planes, every pixel of an inactive tile keeps its bits in every plane
 * asked for; sample_aov entries of inactive sample pixels keep the caller's values; stats->samples = active sample pixels x
 * (sample_end - sample_begin).  All tiles active: the range form bit for bit.  No tile active: PTRS_OK, no launch, planes untouched,
 * zeroed stats.  A row band in params is refused.
 *
 * ptrs_render_aov_adaptive: the planes of a film whose tile t holds tile_spp[t] samples of ptrs_converge_schedule(spp, min_spp) -- what
 * ptrs_render_adaptive returns in tile_spp_out; a pure function of tile_spp, the beauty render is not needed.  Block [begin, end) runs
 * on the tiles with tile_spp[t] >= end; consecutive blocks with the same tile set run as one range, a block without a tile is skipped.
 * The planes stay on the device between the blocks.  Plane k's tile t equals tile t of ptrs_render_aov_range(0, tile_spp[t]) bit for
 * bit; a tile with 0 keeps its bits.  From cleared films, under a pass plan that keeps the band's rows in one pass, every plane's
 * weight equals the weight of the ptrs_render_adaptive film that produced tile_spp, bit for bit on every pixel.  Refused before the
 * first device call: null arguments, a bad planes mask, a row band, an spp or min_spp the schedule refuses, a tile_spp[t] that is
 * neither 0 nor the end of a block (the message names the tile).  stats are summed over the blocks like ptrs_render_adaptive's. */
int ptrs_render_aov_range(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, uint32_t sample_begin, uint32_t sample_end,
                          uint32_t planes, PtrsFilmPixel *const planes_inout[PTRS_AOV_PLANES], float *sample_aov, PtrsStats *stats);
int ptrs_render_aov_range_device(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, uint32_t sample_begin, uint32_t sample_end,
                                 uint32_t planes, void *const planes_inout_device[PTRS_AOV_PLANES], float *sample_aov_device, void *hip_stream, PtrsStats *stats);
int ptrs_render_aov_tiles(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, uint32_t sample_begin, uint32_t sample_end,
                          const uint8_t *tile_active, uint32_t planes, PtrsFilmPixel *const planes_inout[PTRS_AOV_PLANES], float *sample_aov, PtrsStats *stats);
int ptrs_render_aov_tiles_device(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, uint32_t sample_begin, uint32_t sample_end,
                                 const uint8_t *tile_active, uint32_t planes, void *const planes_inout_device[PTRS_AOV_PLANES], float *sample_aov_device,
                                 void *hip_stream, PtrsStats *stats);
int ptrs_render_aov_adaptive(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, uint32_t min_spp, const uint32_t *tile_spp,
                             uint32_t planes, PtrsFilmPixel *const planes_inout[PTRS_AOV_PLANES], PtrsStats *stats);
int ptrs_render_aov_adaptive_device(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, uint32_t min_spp, const uint32_t *tile_spp,
                                    uint32_t planes, void *const planes_inout_device[PTRS_AOV_PLANES], void *hip_stream, PtrsStats *stats);

/* PathIntegrator::render_single_pixel (integrator.rs:505-534): radiance of every sample of one
 * pixel, rgb_out[spp*3]. */
int ptrs_render_single_pixel(PtrsScene *scene, const PtrsCamera *camera,
                             const PtrsRenderParams *params, int32_t px, int32_t py, float *rgb_out);

/* RenderScene::intersect / intersect_p (pathtracer/mod.rs:92-98 -> accelerator.rs:359-475) over a
 * batch of rays, run by the same traversal kernel the renderer uses.
 * rays: n * 7 floats (o.xyz, d.xyz, t_max).  any_hit = 0: closest hit, hits_out = n * PtrsHit.
 * any_hit = 1: hits_out[i].prim = 0 if occluded else -1. */
typedef struct PtrsHit {
    int32_t prim; /* global triangle id (mesh-major), -1 = miss */
    float t;
    float b0, b1, b2; /* barycentrics as computed by Triangle::intersect (shape.rs:157-160) */
} PtrsHit;
int ptrs_trace_rays(PtrsScene *scene, uint32_t n, const float *rays, int32_t any_hit,
                    PtrsHit *hits_out, PtrsStats *stats);

/* Autofocus for a PtrsCameraLens: the pinhole ray of raster point (raster_x, raster_y) is traced with ptrs_trace_rays' closest-hit
 * kernel; *out = t * (-dir_cam.z), dir_cam the normalised camera-space direction: the depth of the hit along the view axis, which is
 * what focal_distance measures.  A miss writes +inf and still returns PTRS_OK. */
int ptrs_camera_focus_distance(PtrsScene *scene, const PtrsCamera *camera, float raster_x, float raster_y, float *out);

/* Traversal bench (the reference's precedent: benches/benchmark_pathtracer.rs:35-54, scene.intersect on one ray in a loop).
 * ptrs_render_dump_rays: starts `params`' render, stops in its first pass before round `round` and returns that round's extension
 * rays (round 0: the camera rays, round k: the rays leaving the paths' k-th vertices), at most max_rays records of 7 floats.
 * ptrs_trace_bench: closest-hit traversal of n rays with the frame's own extension kernel (lane refill, phase voting, persistent
 * waves), `repeats` timed launches after one counting launch: stats->ms_trace (sum of the timed launches), nodes_visited /
 * tris_tested (of ONE launch), rays_extension = n * repeats; hits_out (NULL or n records, t not filled) equals ptrs_trace_rays'. */
int ptrs_render_dump_rays(PtrsScene *scene, const PtrsCamera *camera, const PtrsRenderParams *params, uint32_t round,
                          uint32_t max_rays, float *rays_out, uint32_t *n_out);
int ptrs_trace_bench(PtrsScene *scene, uint32_t n, const float *rays, uint32_t repeats, PtrsHit *hits_out, PtrsStats *stats);

/* SobolSampler (sampler/sobol.rs): value of dimension dims[i] for sample sample_nums[i] of pixel
 * (px[i],py[i]) with the sampler built for `params` -- the device implementation of
 * start_pixel + get_index_for_sample + sample_dimension (81-114,169-193). */
int ptrs_sobol_samples(const PtrsRenderParams *params, uint32_t n, const int32_t *px,
                       const int32_t *py, const uint64_t *sample_nums, const uint32_t *dims,
                       float *out, uint64_t *index_out /* may be NULL */);

/* Self-test of the device code's shared-divisor division (csrc/pt_vec.h, div_shared3: one reciprocal for three quotients -- measured,
 * slower than the compiler's division in the shade kernels and therefore NOT on the render path; the reference divides component by
 * component, e.g. integrator.rs:63-75, 453-497) against the compiler's IEEE division, bit for bit, over
 * about n_sets generated operand sets (a0, a1, a2, b).  mode 0 random bit patterns, 1 exponent / mantissa edge cases, 2 render ranges,
 * 3 Russian-roulette ranges, 4 quotients next to 1 and to rounding ties.  first_bad_out (NULL or 10 words): a0 a1 a2 b, the three
 * quotients computed, the three expected. */
int ptrs_selftest_div3(int32_t device, uint32_t mode, uint64_t n_sets, uint64_t seed, uint64_t *mismatches_out,
                       uint64_t *fast_path_sets_out /* may be NULL */, uint32_t *first_bad_out /* may be NULL */);

/* Known-answer probes (test entry points; the render path does not use them).  They run the device code's
 * csrc/pt_probe.h, one row per thread, at most PTRS_PROBE_MAX_ROWS rows per call.
 * ptrs_probe_bsdf: material `material` of the scene (Matte, Metal, Mirror, Glass, Disney or Substrate, constant
 * textures) at a hit with frame[9] = geometric normal, shading normal, shading dpdu (orthogonal to the shading
 * normal).  rows: n x 8 floats (wo.xyz, wi.xyz, u.xy, world space); out: n x 16 floats = bsdf.f(wo, wi).rgb,
 * bsdf.pdf(wo, wi), sample_f(wo, u): f.rgb, pdf, wi.xyz, sampled flags, then 1 when the material yields a BSDF
 * (0: no BSDF, Q17), 0, 0, 0.
 * ptrs_probe_light: light `light` of the scene, area (triangle) or environment, seen from ref[6] = point, normal.
 * rows: n x 5 floats (u.xy, w.xyz); out: n x 16 floats = sample_li(u): wi.xyz, pdf, Li.rgb, ok; pdf_li(w); le(w).rgb;
 * 0, 0, 0, 0. */
#define PTRS_PROBE_MAX_ROWS (1u << 24)
int ptrs_probe_bsdf(PtrsScene *scene, int32_t material, const float *frame, uint32_t n, const float *rows, float *out);
int ptrs_probe_light(PtrsScene *scene, int32_t light, const float *ref, uint32_t n, const float *rows, float *out);
/* ptrs_probe_texture: texture `tex` of the scene (any kind) through the shade stage's tex_eval.  rows: n x 6 floats (uv.xy, dudx, dvdx,
 * dudy, dvdy); out: n x 8 floats = rgb (1-channel textures in r), then for image textures the MIP level computed from the mapped width,
 * 1 when the zero-footprint shortcut applies, the mapped st.xy, 0.
 * ptrs_probe_surface: triangle `prim` of the scene (mesh order) against one ray per row, then the hit surface of the shade stage
 * (tri_surface, surface_differentials, normal mapping for NormalMaterial wrappers).  rows: n x 16 floats (o.xyz, d.xyz, t_max,
 * rx_d.xyz, ry_d.xyz, w.xyz); out: n x 64 floats in the layout of csrc/pt_probe.h surface_probe_row. */
int ptrs_probe_texture(PtrsScene *scene, int32_t tex, uint32_t n, const float *rows, float *out);
int ptrs_probe_surface(PtrsScene *scene, int32_t prim, uint32_t n, const float *rows, float *out);
/* ptrs_probe_math: the arithmetic substrate itself on device `device`, one function call per row, no scene.  rows: n x 16 floats,
 * out: n x 16 floats, raw results (an integer travels as the bit pattern of a float), unused columns 0.  A NULL buffer, n == 0, an
 * unknown op or more than PTRS_PROBE_MAX_ROWS rows are refused before a device is touched.  op (csrc/pt_probe.h math_probe_row):
 *   0 pt_sinf  1 pt_cosf  2 pt_sincosf (sin, cos)  3 pt_tanf  4 pt_logf  5 pt_log2f  6 pt_expf  7 pt_powf(in0, in1)
 *   8 pt_atan2f(y = in0, x = in1)  9 pt_acosf  10 in0 / in1  11 sqrt_  12 floor_, ceil_, max0_, clamp_(in0, in1, in2)
 *   13 max_, min_  14 max_nz, min_nz  15 (float)bits(in0) * 2^-32, then min_nz(1 - eps, .)
 *   16 f2i_sat(in0), inc_wrap(bits(in1)), abs_mod(bits(in2), bits(in3))
 *   17 next_float_up(in0), next_float_down(in0), gamma_err(bits(in1)), power_heuristic(in2, in3)
 *   18 solve_2x2(in0..3, in4, in5): solved, x0, x1
 *   19 v = in0..2: normalize, coordinate_system v2, v3, spherical_theta, spherical_phi
 *   20 p, p_error, n, w (in0..11): offset_ray_origin, spawn_pair plus, minus, spawn_from
 *   21 u = in0, size = bits(in1) in 2..14, cdf = in2..: find_interval_cdf, find_interval_cdf_guided (guide table built from the cdf) */
int ptrs_probe_math(int32_t device, uint32_t op, uint32_t n, const float *rows, float *out);
/* ptrs_probe_shade_tables (device only): the shade kernels' workgroup tables -- the round's Sobol' window in nibble form, the triangle and
 * light records, the environment light's marginal tables -- staged into LDS arrays of the shade kernels' sizes exactly as round `it` of
 * a render of `scene` with `params` stages them (the sampler, the feature set and the staging configuration come from the render
 * path's own code; nothing is rendered), then one row per thread through that context.  Rows are 12 32-bit words in, 12 out.
 * header_out receives 12 words: sob_lo, sob_n (the window is dimensions [sob_lo, sob_lo + sob_n)), sob_nib (index nibbles staged per
 * dimension: 8 or 13), tri_lds (1: the triangle records are staged), n_lights_lds (light records staged), marg_li (the environment light
 * whose marginal tables the shade kernels stage, 0xffffffff: none), pre_li (the environment light whose samples are computed ahead of the
 * shade kernels, 0xffffffff: none), the shade kernels' feature set (csrc/pt_texture.h FEAT_*), 1 when the render runs the shade kernels
 * built without the in-kernel environment walk, 0, 0, 0.
 *   op 0, Sobol' draws: row = index low word, index high word, scramble, N (1, 2, 3 or 8), N dimensions (each < 1024), rest unused;
 *         out = the N values of the shade context's batched draw as binary32 bit patterns in words 0..N-1, word 8 = the route taken:
 *         0 the global tables, 1 the 8-nibble run of consecutive dimensions, 2 the general loop over the staged nibbles.
 *   op 1, environment sample: row = u.x, u.y (binary32 in [0, 1)), light index (an environment light of the scene); out = the light's
 *         sample for u with the light record and the marginal tables taken from where the shade kernels take them: wi.xyz, pdf, Li.rgb
 *         (binary32), ok (0 / 1), then 1 when the marginal tables came from LDS.
 * NULL buffers, n == 0, more than PTRS_PROBE_MAX_ROWS rows, an unknown op, an N other than 1, 2, 3, 8, a dimension >= 1024, a u outside
 * [0, 1) and a round `it` above 65535 are refused before a device is touched. */
int ptrs_probe_shade_tables(PtrsScene *scene, const PtrsRenderParams *params, uint32_t it, uint32_t op, uint32_t n, const uint32_t *rows,
                            uint32_t *out, uint32_t *header_out);

#ifdef __cplusplus
}
#endif
#endif /* PTRS_H */
