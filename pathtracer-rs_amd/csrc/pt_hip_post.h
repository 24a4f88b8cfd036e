// pt_hip_post.h -- kernels outside the path loop: the denoiser, the film's error, and the self-test and known-answer probe kernels.
// (Part of ptrs_hip.hip's one translation unit, behind the film and feature-plane kernels.)
#pragma once

// ---- denoiser (pt_denoise.h): prepare, `iterations` a-trous launches over ping / pong, finish ------------------------------------
// No queues, no atomics, nothing to spin on: one thread per pixel, every tap bounds-checked.  The iteration kernel has two forms over
// the same per-pixel function (dn_atrous), which differ in where a tap comes from:
//   k_dn_iter        a workgroup is 64 x 4 pixels, lanes are neighbours in x, every tap is two 16-byte global loads
//   k_dn_iter_lds<S> for step S the rows y = r (mod S) form an image of their own with unit row step: a workgroup stages 64 + 4 S
//                    contiguous columns x DN_TILE_T + 4 lattice rows of colour and guide in LDS and filters 64 x DN_TILE_T outputs
//                    out of it; pixels beyond the image are staged as empty ones.  (64 + 4 S)(T + 4) 32 B: 17 KiB at S = 1, 48 KiB at
//                    S = 16, the largest step instantiated -- beyond it the tile would not leave room for several workgroups on a CU.
enum : int { DN_TILE_W = 64, DN_TILE_T = 8, DN_LDS_MAX_STEP = 16 };
enum : uint32_t { DN_LDS_DEFAULT_STEPS = 0u }; // option denoise_lds = -1: the steps (a bit mask) whose shipped form is the LDS tile (the measurement)

__global__ __launch_bounds__(BLOCK) void k_dn_prepare(uint32_t n, const v4 *__restrict__ B, const v4 *__restrict__ A, const v4 *__restrict__ N, const v4 *__restrict__ D,
                                                      v4 *__restrict__ x, v4 *__restrict__ g, v4 *__restrict__ a, int demodulate) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const DnPixel o = dn_prepare(B[i], A[i], N[i], D[i], demodulate != 0);
    x[i] = o.x; g[i] = o.g; a[i] = o.a;
}

__global__ __launch_bounds__(BLOCK) void k_dn_iter(DnIter it, const v4 *__restrict__ xin, const v4 *__restrict__ gin, v4 *__restrict__ xout) {
    const int32_t px = (int32_t)blockIdx.x * 64 + (int32_t)(threadIdx.x & 63u), py = (int32_t)blockIdx.y * WAVES + (int32_t)(threadIdx.x >> 6);
    if (px >= it.W || py >= it.H) return;
    const uint32_t p = (uint32_t)py * (uint32_t)it.W + (uint32_t)px;
    auto fetch = [&](int dx, int dy, v4 &xq, v4 &gq) -> bool {
        const int32_t qx = px + it.step * dx, qy = py + it.step * dy;
        if (qx < 0 || qx >= it.W || qy < 0 || qy >= it.H) return false;
        const uint32_t q = (uint32_t)qy * (uint32_t)it.W + (uint32_t)qx;
        xq = xin[q]; gq = gin[q];
        return dn_ok(xq);
    };
    xout[p] = dn_atrous(it, xin[p], gin[p], fetch);
}

template <int S>
__global__ __launch_bounds__(BLOCK) void k_dn_iter_lds(DnIter it, const v4 *__restrict__ xin, const v4 *__restrict__ gin, v4 *__restrict__ xout) {
    constexpr int COLS = DN_TILE_W + 4 * S, ROWS = DN_TILE_T + 4;
    __shared__ v4 sx[ROWS * COLS], sg[ROWS * COLS];
    const int32_t r = (int32_t)blockIdx.z, x0 = (int32_t)blockIdx.x * DN_TILE_W, j0 = (int32_t)blockIdx.y * DN_TILE_T; // residue, first column, first lattice row
    if (r + S * j0 >= it.H) return; // (the whole workgroup: no output row)
    for (int idx = (int)threadIdx.x; idx < ROWS * COLS; idx += BLOCK) {
        const int row = idx / COLS, col = idx - row * COLS;
        const int32_t gx = x0 - 2 * S + col, gy = r + S * (j0 - 2 + row);
        v4 xv = mkv4(splat3(0.0f), dn_empty_mark()), gv = mkv4(splat3(0.0f), 0.0f);
        if (gx >= 0 && gx < it.W && gy >= 0 && gy < it.H) { const uint32_t q = (uint32_t)gy * (uint32_t)it.W + (uint32_t)gx; xv = xin[q]; gv = gin[q]; }
        sx[idx] = xv; sg[idx] = gv;
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x & 63u);
    const int32_t px = x0 + lx;
    for (int k = (int)(threadIdx.x >> 6); k < DN_TILE_T; k += WAVES) {
        const int32_t py = r + S * (j0 + k);
        if (px >= it.W || py >= it.H) continue;
        const int c = (k + 2) * COLS + lx + 2 * S;
        auto fetch = [&](int dx, int dy, v4 &xq, v4 &gq) -> bool { const int q = c + dy * COLS + dx * S; xq = sx[q]; gq = sg[q]; return dn_ok(xq); };
        xout[(uint32_t)py * (uint32_t)it.W + (uint32_t)px] = dn_atrous(it, sx[c], sg[c], fetch);
    }
}

__global__ __launch_bounds__(BLOCK) void k_dn_finish(uint32_t n, const v4 *__restrict__ x, const v4 *__restrict__ a, v4 *__restrict__ out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) out[i] = dn_finish(x[i], a[i]);
}

// ---- the film's error against its half film (pt_converge.h) ----------------------------------------------------------
// One workgroup per 16 x 16 tile, one thread per pixel: 32 bytes read per pixel, 8 written per tile.  The 256 errors are summed by the
// stride-halving tree of cv_tile_sum: strides 128 and 64 through LDS, the last six across the lanes of wave 0 (lane i takes lane
// i + off's value: for i < off that is v[i] += v[i + off]; what the lanes beyond off make of it is never read again).  The valid
// counts ride along as integers.  A pixel beyond the image is an empty slot and is never loaded.
__global__ __launch_bounds__(BLOCK) void k_film_error(int32_t W, int32_t H, int32_t tiles_x, const v4 *__restrict__ film, const v4 *__restrict__ half, PtrsTileError *__restrict__ tiles) {
    static_assert(BLOCK == CV_SLOTS, "one thread per slot of a tile");
    __shared__ float v[CV_SLOTS]; __shared__ uint32_t c[CV_SLOTS];
    const uint32_t t = threadIdx.x;
    const int32_t x = (int32_t)(blockIdx.x % (uint32_t)tiles_x) * CV_TILE + (int32_t)(t & 15u), y = (int32_t)(blockIdx.x / (uint32_t)tiles_x) * CV_TILE + (int32_t)(t >> 4);
    CvPixel p; p.e = 0.0f; p.valid = 0u;
    if (x < W && y < H) { const size_t q = (size_t)y * (size_t)W + (size_t)x; p = cv_pixel(film[q], half[q]); }
    v[t] = p.e; c[t] = p.valid;
    __syncthreads();
    if (t < 128u) { v[t] = v[t] + v[t + 128u]; c[t] += c[t + 128u]; }
    __syncthreads();
    if (t < 64u) {
        float e = v[t] + v[t + 64u]; uint32_t n = c[t] + c[t + 64u];
        for (int off = 32; off > 0; off >>= 1) { e = e + __shfl_down(e, off); n += (uint32_t)__shfl_down((int)n, off); }
        if (t == 0u) tiles[blockIdx.x] = cv_tile(e, n);
    }
}

// The tile records -> the summary, one workgroup: every thread keeps the best of its tiles (cv_better: larger error, then lower index)
// and their valid pixels, then a tree over the 256 candidates.  Maximum and integer sum do not depend on the order.
__global__ __launch_bounds__(BLOCK) void k_film_error_summary(const PtrsTileError *__restrict__ tiles, uint32_t n_tiles, uint32_t tiles_x, uint32_t tiles_y, PtrsFilmErrorSummary *__restrict__ out) {
    __shared__ float se[BLOCK]; __shared__ uint32_t si[BLOCK]; __shared__ unsigned long long sn[BLOCK];
    const uint32_t t = threadIdx.x;
    float e = -1.0f; uint32_t idx = 0xffffffffu; unsigned long long n = 0ull; // (any tile beats the start: tile errors are >= 0)
    for (uint32_t i = t; i < n_tiles; i += BLOCK) {
        const PtrsTileError T = tiles[i];
        if (cv_better(T.error, i, e, idx)) { e = T.error; idx = i; }
        n += T.valid;
    }
    se[t] = e; si[t] = idx; sn[t] = n;
    for (uint32_t off = BLOCK / 2u; off > 0u; off >>= 1) {
        __syncthreads();
        if (t < off) {
            if (cv_better(se[t + off], si[t + off], se[t], si[t])) { se[t] = se[t + off]; si[t] = si[t + off]; }
            sn[t] += sn[t + off];
        }
    }
    if (t == 0u) { PtrsFilmErrorSummary s; s.max_tile_error = se[0]; s.worst_tile = si[0]; s.valid_pixels = sn[0]; s.tiles_x = tiles_x; s.tiles_y = tiles_y; *out = s; }
}

// ---- the tile form of a pass (pt_adaptive.h): generate, gather and export for the active film tiles only ------------------
// k_generate with a mask.  The slots stay those of the dense pass (sample x pixels + pixel) and the 64-slot chunks are dealt to the
// segments as k_generate deals them, so nothing behind this kernel re-indexes; a lane whose sample pixel is not active (ad_pixel_active:
// up to four flag bytes) makes no path, and the wave compacts the others into the segment with a ballot (wave_push), so a segment's
// entries stay consecutive and seg_count gets the true number.  With every tile active the queue is k_generate's, entry for entry.
__global__ __launch_bounds__(BLOCK) void k_generate_tiles(DParams R, DSampler S, DCamera C, DPaths P, DQueues Q, uint32_t seg_cap, uint32_t G, uint32_t deal,
                                                          const uint8_t *__restrict__ tile_active, int32_t tiles_x) {
    const uint32_t lane = threadIdx.x & 63u, s = wave_of_launch();
    if (s >= G) return;
    const uint32_t chunks = (R.n_paths + 63u) / 64u;
    const uint32_t e0 = s * seg_cap;
    uint32_t n = 0; // wave-uniform
    auto chunk = [&](uint32_t c) {
        const uint32_t pid = c * 64u + lane;
        bool on = false;
        if (pid < R.n_paths) { const PathCoord pc = path_coord(R, S, pid); on = ad_pixel_active(tile_active, tiles_x, R.W, R.H, pc.px, pc.py); }
        const uint32_t e = e0 + wave_push(n, on); // (at most 64 per chunk, at most seg_cap / 64 chunks per segment: inside the segment)
        if (on) { generate_item(R, S, C, P, pid, e); pslot(Q.ext[0], e) = pid; }
    };
    if (!deal) {
        for (uint32_t c = s; c < chunks; c += G) chunk(c);
    } else { // k_generate's walk by image region
        const uint32_t npix = (uint32_t)(R.row1 - R.row0) * (uint32_t)R.NX;
        uint32_t cpp = (npix + 63u) / 64u;
        if (cpp > chunks) cpp = chunks;
        if (cpp < 1u) cpp = 1u;
        const uint32_t nsr = (chunks + cpp - 1u) / cpp, r_last = chunks - (nsr - 1u) * cpp, full = r_last * nsr, cps = seg_cap / 64u;
        const uint32_t c1 = (s + 1u) * cps < chunks ? (s + 1u) * cps : chunks;
        for (uint32_t cc = s * cps; cc < c1; ++cc) {
            uint32_t pc, k;
            if (cc < full) { pc = cc / nsr; k = cc - pc * nsr; }
            else { const uint32_t d = cc - full, q = d / (nsr - 1u); pc = r_last + q; k = d - q * (nsr - 1u); }
            chunk(k * cpp + pc);
        }
    }
    if (lane == 0) *seg_count(Q, 0, Q_EXT, G, s) = n;
}

// k_film for the active tiles: one workgroup per entry of the list, the tile's origin on the FILM's grid (not y0 + 16 j), clipped to the
// pass's output rows [y0, y1) at both ends -- a tile of the film's grid can straddle y0 of a row-split pass.  Per pixel the sums are
// k_film's in k_film's order (k, then dx, then dy): a pixel's order never depended on where its tile begins.  Only slots of active
// sample pixels are read: an apron entry is staged when it lies within the filter radius of a pixel the tile really has (the tile is
// clipped at the film's right and bottom edges), and such a sample pixel is active by the dilation rule.
__global__ __launch_bounds__(BLOCK) void k_film_tiles(DParams R, DSampler S, DPaths P, const float *__restrict__ table, v4 *film, int32_t y0, int32_t y1, int32_t tiles_x,
                                                      const uint32_t *__restrict__ tile_list) {
    __shared__ float tab[256];
    __shared__ v4 s_a[400]; __shared__ float s_lb[400];
    __shared__ uint32_t s_m[400];
    const uint32_t t = tile_list[blockIdx.x];
    const int32_t tx0 = (int32_t)(t % (uint32_t)tiles_x) * CV_TILE, ty0 = (int32_t)(t / (uint32_t)tiles_x) * CV_TILE;
    if (ty0 >= y1 || ty0 + CV_TILE <= y0) return; // (the whole workgroup: none of the tile's rows is in this pass)
    tab[threadIdx.x] = table[threadIdx.x];
    const int32_t lx = (int32_t)(threadIdx.x & 15u), ly = (int32_t)(threadIdx.x >> 4);
    const FilmTile T{tx0, ty0, lx, ly, tx0 + lx, ty0 + ly, tx0 + lx < R.W && ty0 + ly >= y0 && ty0 + ly < y1, (1u << (uint32_t)lx) | (1u << (16u + (uint32_t)ly))};
    const int32_t ax1 = (tx0 + CV_TILE < R.W ? tx0 + CV_TILE : R.W) + 2, ay1 = (ty0 + CV_TILE < R.H ? ty0 + CV_TILE : R.H) + 2; // the apron the tile's own pixels reach, exclusive
    v4 acc; acc.x = acc.y = acc.z = acc.w = 0.0f;
    if (T.live) acc = film[(size_t)T.y * (size_t)R.W + (size_t)T.x];
    const uint32_t npix = (uint32_t)(R.row1 - R.row0) * (uint32_t)R.NX;
    const uint32_t ns = R.s1 - R.s0;
    for (uint32_t k = 0; k < ns; ++k) {
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < 400u; e += BLOCK) {
            float pfx = -1.0e9f, pfy = -1.0e9f, lr = 0.0f, lg = 0.0f, lb = 0.0f;
            uint32_t pid = 0;
            const bool reached = tx0 - 2 + (int32_t)(e % 20u) < ax1 && ty0 - 2 + (int32_t)(e / 20u) < ay1;
            if (film_apron_pid(R, S, T, e, k, npix, pid) && reached) {
                const f2a pf = pslot(P.pfilm, pid); const v4 Lv = pslot(P.L, pid);
                pfx = pf.x; pfy = pf.y; lr = Lv.x; lg = Lv.y; lb = Lv.z;
            }
            const float pdx = pfx - 0.5f, pdy = pfy - 0.5f;
            s_m[e] = film_footprint_mask(pdx, pdy, T);
            v4 a; a.x = pdx; a.y = pdy; a.z = lr; a.w = lg; s_a[e] = a; s_lb[e] = lb;
        }
        __syncthreads();
        if (T.live) {
            for (int32_t dx = 0; dx < 5; ++dx)
                for (int32_t dy = 0; dy < 5; ++dy) {
                    const int32_t e = (T.ly + dy) * 20 + (T.lx + dx);
                    if ((s_m[e] & T.my_bits) != T.my_bits) continue;
                    const v4 a = s_a[e];
                    const float w = film_weight_inside(a.x, a.y, T.x, T.y, tab);
                    acc.x += a.z * w; acc.y += a.w * w; acc.z += s_lb[e] * w; acc.w += w;
                }
        }
    }
    if (T.live) film[(size_t)T.y * (size_t)R.W + (size_t)T.x] = acc;
}

// k_export_samples for the active sample pixels: the entries of the others keep what the caller's buffer held
__global__ __launch_bounds__(BLOCK) void k_export_samples_tiles(DParams R, DSampler S, DPaths P, float *out, const uint8_t *__restrict__ tile_active, int32_t tiles_x) {
    const uint32_t stride = gridDim.x * BLOCK;
    for (uint32_t pid = blockIdx.x * BLOCK + threadIdx.x; pid < R.n_paths; pid += stride) {
        const PathCoord c = path_coord(R, S, pid);
        if (!ad_pixel_active(tile_active, tiles_x, R.W, R.H, c.px, c.py)) continue;
        const size_t o = (((size_t)c.sy * (size_t)R.NX + (size_t)c.sx) * S.spp + c.s) * 3;
        const v4 L = pslot(P.L, pid);
        out[o] = L.x; out[o + 1] = L.y; out[o + 2] = L.z;
    }
}

// ---- the tile form of an AOV pass (pt_aov.h): k_generate_tiles and k_aov as they stand, then these two ----------------------
// k_film_aov's three-accumulator gather with k_film_tiles' placement: one workgroup per entry of the list, the tile's origin on the film's
// grid, clipped to [y0, y1), and the `reached` test on every apron entry.  That test is what keeps the kernel off STALE slots: k_aov
// walks the queue k_generate_tiles made, so the value arrays (and in band mode the band's p_film copy) are written for active sample
// pixels only; every other slot holds what an earlier pass, sample index or call left there.  An apron entry is read only when it is
// within the filter radius of a pixel the tile really has, and such a sample pixel is active by the dilation rule (ad_pixel_active).
// Per pixel the additions are k_film_aov's in its order (k, dx, dy).  LDS as k_film_aov: 3 x 400 x 16 + 400 x 4 + 1024 bytes.
__global__ __launch_bounds__(BLOCK) void k_film_aov_tiles(DParams R, DSampler S, DPaths P, DAov A, const float *__restrict__ table, DAovFilm F, int32_t y0, int32_t y1, int32_t tiles_x,
                                                          const uint32_t *__restrict__ tile_list) {
    __shared__ float tab[256];
    __shared__ v4 s_p[400], s_al[400], s_n[400]; // p_film.xy - 0.5, depth, coverage | albedo.rgb | normal.rgb
    __shared__ uint32_t s_m[400];
    const uint32_t t = tile_list[blockIdx.x];
    const int32_t tx0 = (int32_t)(t % (uint32_t)tiles_x) * CV_TILE, ty0 = (int32_t)(t / (uint32_t)tiles_x) * CV_TILE;
    if (ty0 >= y1 || ty0 + CV_TILE <= y0) return; // (the whole workgroup: none of the tile's rows is in this gather)
    tab[threadIdx.x] = table[threadIdx.x];
    const int32_t lx = (int32_t)(threadIdx.x & 15u), ly = (int32_t)(threadIdx.x >> 4);
    const FilmTile T{tx0, ty0, lx, ly, tx0 + lx, ty0 + ly, tx0 + lx < R.W && ty0 + ly >= y0 && ty0 + ly < y1, (1u << (uint32_t)lx) | (1u << (16u + (uint32_t)ly))};
    const int32_t ax1 = (tx0 + CV_TILE < R.W ? tx0 + CV_TILE : R.W) + 2, ay1 = (ty0 + CV_TILE < R.H ? ty0 + CV_TILE : R.H) + 2; // the apron the tile's own pixels reach, exclusive
    const bool want_al = F.plane[AOV_ALBEDO] != nullptr, want_n = F.plane[AOV_NORMAL] != nullptr, want_d = F.plane[AOV_DEPTH] != nullptr;
    const size_t px = (size_t)T.y * (size_t)R.W + (size_t)T.x;
    v4 acc_al, acc_n, acc_d;
    acc_al.x = acc_al.y = acc_al.z = acc_al.w = 0.0f; acc_n = acc_al; acc_d = acc_al;
    if (T.live) {
        if (want_al) acc_al = F.plane[AOV_ALBEDO][px];
        if (want_n) acc_n = F.plane[AOV_NORMAL][px];
        if (want_d) acc_d = F.plane[AOV_DEPTH][px];
    }
    const uint32_t npix = (uint32_t)(R.row1 - R.row0) * (uint32_t)R.NX;
    const uint32_t ns = R.s1 - R.s0;
    for (uint32_t k = 0; k < ns; ++k) {
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < 400u; e += BLOCK) {
            float pfx = -1.0e9f, pfy = -1.0e9f;
            v4 al, nd; al.x = al.y = al.z = al.w = 0.0f; nd = al;
            uint32_t pid = 0;
            const bool reached = tx0 - 2 + (int32_t)(e % 20u) < ax1 && ty0 - 2 + (int32_t)(e / 20u) < ay1;
            if (film_apron_pid(R, S, T, e, k, npix, pid) && reached) {
                const f2a pf = pslot(P.pfilm, pid);
                pfx = pf.x; pfy = pf.y; al = pslot(A.albedo, pid); nd = pslot(A.normal, pid);
            }
            const float pdx = pfx - 0.5f, pdy = pfy - 0.5f;
            s_m[e] = film_footprint_mask(pdx, pdy, T);
            v4 a; a.x = pdx; a.y = pdy; a.z = nd.w; a.w = al.w; s_p[e] = a; s_al[e] = al; s_n[e] = nd;
        }
        __syncthreads();
        if (T.live) {
            for (int32_t dx = 0; dx < 5; ++dx)
                for (int32_t dy = 0; dy < 5; ++dy) {
                    const int32_t e = (T.ly + dy) * 20 + (T.lx + dx);
                    if ((s_m[e] & T.my_bits) != T.my_bits) continue;
                    const v4 a = s_p[e];
                    const float w = film_weight_inside(a.x, a.y, T.x, T.y, tab);
                    if (want_al) { const v4 c = s_al[e]; acc_al.x += c.x * w; acc_al.y += c.y * w; acc_al.z += c.z * w; acc_al.w += w; }
                    if (want_n) { const v4 c = s_n[e]; acc_n.x += c.x * w; acc_n.y += c.y * w; acc_n.z += c.z * w; acc_n.w += w; }
                    if (want_d) { acc_d.x += a.z * w; acc_d.y += a.w * w; acc_d.z += 0.0f * w; acc_d.w += w; }
                }
        }
    }
    if (T.live) {
        if (want_al) F.plane[AOV_ALBEDO][px] = acc_al;
        if (want_n) F.plane[AOV_NORMAL][px] = acc_n;
        if (want_d) F.plane[AOV_DEPTH][px] = acc_d;
    }
}

// k_export_aov for the active sample pixels: the entries of the others keep what the caller's buffer held
__global__ __launch_bounds__(BLOCK) void k_export_aov_tiles(DParams R, DSampler S, DAov A, uint32_t off, float *out, const uint8_t *__restrict__ tile_active, int32_t tiles_x) {
    const uint32_t stride = gridDim.x * BLOCK;
    for (uint32_t pid = blockIdx.x * BLOCK + threadIdx.x; pid < R.n_paths; pid += stride) {
        const PathCoord c = path_coord(R, S, pid);
        if (!ad_pixel_active(tile_active, tiles_x, R.W, R.H, c.px, c.py)) continue;
        float *o = out + (((size_t)c.sy * (size_t)R.NX + (size_t)c.sx) * S.spp + c.s) * AOV_SAMPLE_FLOATS;
        const v4 al = pslot(A.albedo, off + pid), nd = pslot(A.normal, off + pid), pp = pslot(A.pos, off + pid);
        o[0] = al.x; o[1] = al.y; o[2] = al.z; o[3] = al.w;
        o[4] = nd.x; o[5] = nd.y; o[6] = nd.z; o[7] = nd.w;
        o[8] = pp.x; o[9] = pp.y; o[10] = pp.z; o[11] = pp.w;
    }
}

__global__ __launch_bounds__(BLOCK) void k_sobol(DSampler S, uint32_t n, const int32_t *px, const int32_t *py, const uint64_t *sn, const uint32_t *dims, float *out, uint64_t *idx_out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t idx = sobol_index(S, sn[i], (uint32_t)(px[i] - S.min_x), (uint32_t)(py[i] - S.min_y));
    if (idx_out) idx_out[i] = idx;
    out[i] = sample_dimension(S, idx, dims[i], pixel_scramble(px[i], py[i]), px[i], py[i]);
}

// Self-test of the shared-divisor division (pt_vec.h, div_shared3) against the compiler's IEEE division, bit for bit, on
// operand sets drawn from a counter-based generator.  mode 0: raw random bit patterns (every class at its natural share: 1/256 each of
// zeros + denormals and infinities + NaNs); 1: exponents around every threshold of the fast path's window and of v_div_scale /
// v_div_fixup, mantissas random / all zeros / all ones, signed zeros; 2: the ranges of a render (pdf-like divisors 2^-27 .. 2^13,
// radiance-like numerators, a quarter of them zero); 3: beta / (1 - q) of the Russian roulette; 4: quotients next to 1 and next to
// rounding ties (a = b x small factors, a = b +- ulps).
__device__ inline uint64_t mix64(uint64_t z) { z += 0x9e3779b97f4a7c15ull; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
__device__ inline uint32_t edge_bits(uint32_t r) { // r: 32 random bits
    const uint32_t exps[32] = {0, 0, 1, 2, 22, 23, 24, 25, 31, 32, 33, 78, 79, 80, 81, 82, 126, 127, 128, 150, 172, 173, 174, 175, 176, 221, 222, 223, 252, 253, 254, 255};
    const uint32_t e = exps[r & 31u], how = (r >> 5) & 3u, sign = (r >> 7) & 1u;
    const uint32_t man = how == 0u ? 0u : (how == 1u ? 0x7fffffu : ((r >> 9) & 0x7fffffu));
    return (sign << 31) | (e << 23) | man;
}
__global__ __launch_bounds__(BLOCK) void k_selftest_div3(uint64_t seed, uint32_t mode, uint64_t per_thread, unsigned long long *out /* [0] mismatches, [1] fast-path sets */, uint32_t *first_bad /* 10 words + a lock */) {
    const uint64_t tid = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    unsigned long long bad = 0, fast = 0;
    for (uint64_t k = 0; k < per_thread; ++k) {
        const uint64_t h0 = mix64(seed ^ (tid * per_thread + k) * 0xd1342543de82ef95ull), h1 = mix64(h0);
        uint32_t w[4] = {(uint32_t)h0, (uint32_t)(h0 >> 32), (uint32_t)h1, (uint32_t)(h1 >> 32)};
        if (mode == 1u) { for (int j = 0; j < 4; ++j) w[j] = edge_bits(w[j]); }
        else if (mode == 2u) {
            w[3] = ((100u + (w[3] >> 24) % 41u) << 23) | (w[3] & 0x7fffffu);
            for (int j = 0; j < 3; ++j) w[j] = (w[j] >> 30) == 0u ? (w[j] & 0x80000000u) : (((90u + (w[j] >> 24) % 51u) << 23) | (w[j] & 0x7fffffu) | ((w[j] >> 29) == 7u ? 0x80000000u : 0u));
        } else if (mode == 3u) {
            const float mx = (float)(w[3] >> 8) * 0x1p-24f;
            const float q = max_nz(0.05f, 1.0f - mx);
            w[3] = f2u(1.0f - q);
            for (int j = 0; j < 3; ++j) w[j] = f2u((float)(w[j] >> 8) * 0x1p-23f * ((w[j] & 255u) == 0u ? 0.0f : 1.0f));
        } else if (mode == 4u) {
            const uint32_t b = ((80u + (w[3] >> 24) % 90u) << 23) | (w[3] & 0x7fffffu) | ((w[3] >> 23 & 1u) << 31);
            w[3] = b;
            for (int j = 0; j < 3; ++j) {
                const uint32_t sel = w[j] & 7u, d = (w[j] >> 3) & 15u;
                const float fb = u2f(b);
                float a = fb;
                if (sel == 0u) a = u2f(b + d); else if (sel == 1u) a = u2f(b - d); else if (sel == 2u) a = fb * (float)(1u + d); else if (sel == 3u) a = fb * (1.0f + (float)d * 0x1p-23f);
                else if (sel == 4u) a = fb * 0x1.fffffep-1f; else if (sel == 5u) a = fb * 0.5f + u2f((f2u(fb) & 0xff800000u) - (12u << 23)); else if (sel == 6u) a = u2f((b & 0xff800000u) | 0x7fffffu); else a = u2f(b & 0xff800000u);
                w[j] = f2u(a);
            }
        }
        const float ax = u2f(w[0]), ay = u2f(w[1]), az = u2f(w[2]), b = u2f(w[3]);
        const f3 got = div_shared3(mk3(ax, ay, az), b);
        const float wx = ax / b, wy = ay / b, wz = az / b; // the compiler's IEEE division
        { // (how many sets took the fast path: the test wants to know that it was exercised)
            const uint32_t LO = 80u << 23, HI = 175u << 23, ux = w[0] & 0x7fffffffu, uy = w[1] & 0x7fffffffu, uz = w[2] & 0x7fffffffu, us = w[3] & 0x7fffffffu;
            auto okn = [&](uint32_t u) { return u == 0u || (u >= LO && u < HI); };
            if (us >= LO && us < HI && okn(ux) && okn(uy) && okn(uz)) ++fast;
        }
        if (f2u(got.x) != f2u(wx) || f2u(got.y) != f2u(wy) || f2u(got.z) != f2u(wz)) {
            ++bad;
            if (atomicCAS(first_bad + 10, 0u, 1u) == 0u) { first_bad[0] = w[0]; first_bad[1] = w[1]; first_bad[2] = w[2]; first_bad[3] = w[3]; first_bad[4] = f2u(got.x); first_bad[5] = f2u(got.y); first_bad[6] = f2u(got.z); first_bad[7] = f2u(wx); first_bad[8] = f2u(wy); first_bad[9] = f2u(wz); }
        }
    }
    if (bad) atomicAdd(out, bad);
    atomicAdd(out + 1, fast);
}

// Known-answer probes (csrc/pt_probe.h): one row per thread, the same functions the host twin runs.
struct ProbeArgs { float v[9]; }; // BSDF: ng, ns, dpdu; light: p, n (6 used)
__global__ __launch_bounds__(BLOCK) void k_probe_bsdf(DScene sc, int32_t mat, int32_t kind, ProbeArgs frame, uint32_t n, const float *__restrict__ in, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    bsdf_probe_row(sc, mat, kind, frame.v, in + (uint64_t)i * PROBE_BSDF_IN, out + (uint64_t)i * PROBE_BSDF_OUT);
}
__global__ __launch_bounds__(BLOCK) void k_probe_light(DScene sc, int32_t light, ProbeArgs ref, uint32_t n, const float *__restrict__ in, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    light_probe_row(sc, light, ref.v, in + (uint64_t)i * PROBE_LIGHT_IN, out + (uint64_t)i * PROBE_LIGHT_OUT);
}

__global__ __launch_bounds__(BLOCK) void k_probe_texture(DScene sc, int32_t tex, uint32_t n, const float *__restrict__ in, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    texture_probe_row(sc, tex, in + (uint64_t)i * PROBE_TEX_IN, out + (uint64_t)i * PROBE_TEX_OUT);
}
__global__ __launch_bounds__(BLOCK) void k_probe_surface(DScene sc, uint32_t prim, uint32_t n, const float *__restrict__ in, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    surface_probe_row(sc, prim, in + (uint64_t)i * PROBE_SURF_IN, out + (uint64_t)i * PROBE_SURF_OUT);
}
__global__ __launch_bounds__(BLOCK) void k_probe_math(uint32_t op, uint32_t n, const float *__restrict__ in, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    math_probe_row(op, in + (uint64_t)i * PROBE_MATH_IN, out + (uint64_t)i * PROBE_MATH_OUT);
}

// The shade stage's LDS context at rows of the test's choosing (ptrs_probe_shade_tables): the tables staged by stage_shade_tables into
// arrays of the shade kernels' sizes, the barrier, then one row per thread through ShadeCtxLds.  MARG: the instantiations that stage the
// environment light's marginal tables (scenes with FEAT_INFINITE); the staging code does not depend on the feature set otherwise.
template <int N>
__device__ inline void probe_shade_sobol_row(const ShadeCtxLds<false> &X, const DSampler &S, const uint32_t *in, uint32_t *out) {
    const uint64_t index = (uint64_t)in[0] | ((uint64_t)in[1] << 32);
    uint32_t dim[N], route = 0xffffffffu;
    float v[N];
    for (int k = 0; k < N; ++k) dim[k] = in[4 + k];
    X.template sobol<N, true>(S, index, dim, in[2], v, &route);
    for (int k = 0; k < N; ++k) out[k] = f2u(v[k]);
    out[8] = route;
}
template <bool MARG>
__global__ __launch_bounds__(BLOCK) void k_probe_shade(DSampler S, DScene sc, ShadeLdsCfg cfg, uint32_t op, uint32_t n, const uint32_t *__restrict__ in, uint32_t *__restrict__ out) {
    __shared__ uint32_t lds_sob[SH_SOB_WORDS];
    __shared__ v4 lds_tri[SH_TRI_V4];
    __shared__ v4 lds_light[SH_LIGHTS * SH_LIGHT_V4];
    __shared__ float lds_marg[MARG ? SH_MARG_WORDS : 1];
    const ShadeCtxLds<false> X = stage_shade_tables<MARG ? FEAT_IMG_ENV : FEAT_SIMPLE, false>(S, sc, cfg, lds_sob, lds_tri, lds_light, lds_marg);
    __syncthreads();
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t *r = in + (uint64_t)i * PROBE_SHADE_IN;
    uint32_t *o = out + (uint64_t)i * PROBE_SHADE_OUT;
    for (uint32_t k = 0; k < PROBE_SHADE_OUT; ++k) o[k] = 0u;
    if (op == PROBE_SHADE_SOBOL) {
        switch (r[3]) { // (the entry point has checked N)
            case 1: probe_shade_sobol_row<1>(X, S, r, o); break;
            case 2: probe_shade_sobol_row<2>(X, S, r, o); break;
            case 3: probe_shade_sobol_row<3>(X, S, r, o); break;
            default: probe_shade_sobol_row<8>(X, S, r, o); break;
        }
    } else { // PROBE_SHADE_ENV: the light's record and its marginal tables from where shade_item takes them
        const uint32_t li = r[2];
        DLight Lt;
        X.light(sc, li, Lt);
        f3 wi, rgb; float pdf;
        const bool ok = inf_light_sample(sc, Lt, mk2(u2f(r[0]), u2f(r[1])), wi, pdf, rgb, X.inf_marginal(li));
        o[0] = f2u(wi.x); o[1] = f2u(wi.y); o[2] = f2u(wi.z); o[3] = f2u(pdf); o[4] = f2u(rgb.x); o[5] = f2u(rgb.y); o[6] = f2u(rgb.z); o[7] = ok ? 1u : 0u;
        o[8] = X.inf_marginal(li) ? 1u : 0u;
    }
}
