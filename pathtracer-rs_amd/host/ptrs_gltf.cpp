// ptrs_gltf.cpp -- glTF 2.0 branch of importer::import for the C++ host.  Restates
//   common/importer/gltf.rs:3-117        camera search, default camera, node transforms
//   pathtracer/importer/gltf.rs:20-584   materials, meshes, emissive area lights, punctual lights, default env light
//   pathtracer/texture.rs:97-177,279-405 ImageTexture constructors and the MIP pyramid they build
//   pathtracer/light.rs:331-398          InfiniteAreaLight::new (RGBE map, Distribution2D)
// in the arithmetic order of pathtracer-rs_amd/{gltf,textures}.py, so both hosts hand the C ABI the same bits
// (tests/test_host_cpp.py).  Third-party behaviour (gltf 1.1.0, image 0.23.14, nalgebra-glm) is restated from the
// crates' published semantics: parity unpinned, see DESIGN.md.  Images: PNG (own inflate-based decoder) and baseline
// JPEG (own decoder, within a level or two of other decoders).  The quirks listed at the top of gltf.py are kept here as well.
#include <zlib.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>

#include "ptrs_host.hpp"

namespace ptrs_host {
namespace {

// ---- JSON -----------------------------------------------------------------------------------------------
struct JVal {
    enum Type { Null, Bool, Num, Str, Arr, Obj } type = Null;
    bool b = false; double n = 0.0; std::string s;
    std::vector<JVal> a;
    std::vector<std::pair<std::string, JVal>> o;
    const JVal *get(const char *k) const { if (type != Obj) return nullptr; for (auto &kv : o) if (kv.first == k) return &kv.second; return nullptr; }
    bool has(const char *k) const { return get(k) != nullptr; }
    double num(const char *k, double def) const { const JVal *v = get(k); return v && v->type == Num ? v->n : def; }
    int integer(const char *k, int def) const { const JVal *v = get(k); return v && v->type == Num ? (int)v->n : def; }
    std::string str(const char *k, const std::string &def = "") const { const JVal *v = get(k); return v && v->type == Str ? v->s : def; }
    size_t size() const { return type == Arr ? a.size() : 0; }
    const JVal &at(size_t i) const { return a[i]; }
};
struct JParser {
    const std::string &s; size_t i = 0; std::string err;
    explicit JParser(const std::string &src) : s(src) {}
    void ws() { while (i < s.size() && (s[i] == ' ' || s[i] == '\n' || s[i] == '\r' || s[i] == '\t')) ++i; }
    bool fail(const char *m) { if (err.empty()) err = std::string(m) + " at byte " + std::to_string(i); return false; }
    bool value(JVal &v, int depth = 0) {
        if (depth > 200) return fail("nesting too deep");
        ws();
        if (i >= s.size()) return fail("unexpected end");
        const char c = s[i];
        if (c == '{') {
            v.type = JVal::Obj; ++i; ws();
            if (i < s.size() && s[i] == '}') { ++i; return true; }
            for (;;) {
                ws(); JVal k; if (i >= s.size() || s[i] != '"' || !string(k.s)) return fail("object key expected");
                ws(); if (i >= s.size() || s[i] != ':') return fail("':' expected"); ++i;
                JVal x; if (!value(x, depth + 1)) return false;
                v.o.emplace_back(std::move(k.s), std::move(x));
                ws(); if (i < s.size() && s[i] == ',') { ++i; continue; }
                if (i < s.size() && s[i] == '}') { ++i; return true; }
                return fail("',' or '}' expected");
            }
        }
        if (c == '[') {
            v.type = JVal::Arr; ++i; ws();
            if (i < s.size() && s[i] == ']') { ++i; return true; }
            for (;;) {
                JVal x; if (!value(x, depth + 1)) return false;
                v.a.push_back(std::move(x));
                ws(); if (i < s.size() && s[i] == ',') { ++i; continue; }
                if (i < s.size() && s[i] == ']') { ++i; return true; }
                return fail("',' or ']' expected");
            }
        }
        if (c == '"') { v.type = JVal::Str; return string(v.s); }
        if (s.compare(i, 4, "true") == 0) { v.type = JVal::Bool; v.b = true; i += 4; return true; }
        if (s.compare(i, 5, "false") == 0) { v.type = JVal::Bool; v.b = false; i += 5; return true; }
        if (s.compare(i, 4, "null") == 0) { v.type = JVal::Null; i += 4; return true; }
        char *end = nullptr;
        v.n = std::strtod(s.c_str() + i, &end);
        if (end == s.c_str() + i) return fail("value expected");
        v.type = JVal::Num; i = (size_t)(end - s.c_str());
        return true;
    }
    bool string(std::string &out) {
        ++i; // opening quote
        while (i < s.size() && s[i] != '"') {
            if (s[i] == '\\' && i + 1 < s.size()) {
                const char e = s[i + 1]; i += 2;
                switch (e) {
                    case 'n': out += '\n'; break; case 't': out += '\t'; break; case 'r': out += '\r'; break;
                    case 'b': out += '\b'; break; case 'f': out += '\f'; break;
                    case 'u': { if (i + 4 > s.size()) return fail("bad \\u escape"); unsigned cp = (unsigned)std::strtoul(s.substr(i, 4).c_str(), nullptr, 16); i += 4;
                                if (cp < 0x80) out += (char)cp; else if (cp < 0x800) { out += (char)(0xC0 | (cp >> 6)); out += (char)(0x80 | (cp & 0x3F)); }
                                else { out += (char)(0xE0 | (cp >> 12)); out += (char)(0x80 | ((cp >> 6) & 0x3F)); out += (char)(0x80 | (cp & 0x3F)); } break; }
                    default: out += e;
                }
            } else out += s[i++];
        }
        if (i >= s.size()) return fail("unterminated string");
        ++i;
        return true;
    }
};

bool read_file(const std::string &path, std::string &out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    return true;
}
std::string base64_decode(const std::string &in) {
    std::string out; unsigned acc = 0; int bits = 0;
    for (unsigned char c : in) {
        int v;
        if (c >= 'A' && c <= 'Z') v = c - 'A'; else if (c >= 'a' && c <= 'z') v = c - 'a' + 26; else if (c >= '0' && c <= '9') v = c - '0' + 52;
        else if (c == '+' || c == '-') v = 62; else if (c == '/' || c == '_') v = 63; else continue;
        acc = (acc << 6) | (unsigned)v; bits += 6;
        if (bits >= 8) { bits -= 8; out += (char)((acc >> bits) & 0xFF); }
    }
    return out;
}
std::string dir_of(const std::string &p) { size_t k = p.find_last_of('/'); return k == std::string::npos ? "." : p.substr(0, k); }

// ---- PNG decoder (8/16-bit, colour types 0/2/3/4/6, non-interlaced) -> channels as image 0.23 reports them --------
struct Image8 { int w = 0, h = 0, ch = 0; std::vector<uint8_t> px; bool supported = false; };
bool decode_png(const std::string &d, Image8 &img, std::string &err) {
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (d.size() < 8 || std::memcmp(d.data(), sig, 8) != 0) { err = "unknown image format"; return false; }
    auto be32 = [&](size_t o) { return ((uint32_t)(uint8_t)d[o] << 24) | ((uint32_t)(uint8_t)d[o + 1] << 16) | ((uint32_t)(uint8_t)d[o + 2] << 8) | (uint32_t)(uint8_t)d[o + 3]; };
    size_t o = 8; uint32_t w = 0, h = 0; int depth = 0, ctype = 0, interlace = 0;
    std::string idat; std::vector<uint8_t> plte, trns;
    while (o + 12 <= d.size()) {
        const uint32_t n = be32(o); const std::string tag = d.substr(o + 4, 4);
        if (o + 12 + n > d.size()) { err = "truncated PNG"; return false; }
        const char *p = d.data() + o + 8;
        if (tag == "IHDR") { w = be32(o + 8); h = be32(o + 12); depth = (uint8_t)p[8]; ctype = (uint8_t)p[9]; interlace = (uint8_t)p[12]; }
        else if (tag == "PLTE") plte.assign(p, p + n);
        else if (tag == "tRNS") trns.assign(p, p + n);
        else if (tag == "IDAT") idat.append(p, n);
        else if (tag == "IEND") break;
        o += 12 + n;
    }
    if (!w || !h || interlace) { err = "unsupported PNG (interlaced or empty)"; return false; }
    const int nch = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
    if (!nch || (depth != 8 && depth != 16 && !(depth < 8 && (ctype == 0 || ctype == 3)))) { err = "unsupported PNG colour type / depth"; return false; }
    const size_t bpp_bits = (size_t)nch * depth, stride = (w * bpp_bits + 7) / 8, bpp = std::max<size_t>(1, bpp_bits / 8);
    std::vector<uint8_t> raw((stride + 1) * h);
    uLongf rl = (uLongf)raw.size();
    if (uncompress(raw.data(), &rl, (const Bytef *)idat.data(), (uLong)idat.size()) != Z_OK || rl != raw.size()) { err = "PNG inflate failed"; return false; }
    std::vector<uint8_t> cur(stride), prev(stride, 0), rows(stride * h);
    for (uint32_t y = 0; y < h; ++y) {
        const uint8_t *in = &raw[(stride + 1) * y]; const int ft = in[0]; ++in;
        for (size_t x = 0; x < stride; ++x) {
            const int a = x >= bpp ? cur[x - bpp] : 0, b = prev[x], c = x >= bpp ? prev[x - bpp] : 0;
            int pr = 0;
            switch (ft) {
                case 0: pr = 0; break; case 1: pr = a; break; case 2: pr = b; break; case 3: pr = (a + b) >> 1; break;
                case 4: { const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c); pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); break; }
                default: err = "bad PNG filter"; return false;
            }
            cur[x] = (uint8_t)(in[x] + pr);
        }
        std::memcpy(&rows[stride * y], cur.data(), stride);
        prev = cur;
    }
    auto sample = [&](uint32_t y, size_t idx) -> unsigned { // idx-th sample of row y, reduced to 8 bits (palette index kept as is)
        const uint8_t *r = &rows[stride * y];
        if (depth == 8) return r[idx];
        if (depth == 16) return r[2 * idx];
        const unsigned per = 8u / (unsigned)depth, v = (r[idx / per] >> ((per - 1 - idx % per) * depth)) & ((1u << depth) - 1u);
        return ctype == 3 ? v : v * 255u / ((1u << depth) - 1u);
    };
    img.w = (int)w; img.h = (int)h;
    if (ctype == 3) { // palette -> RGB8 (RGBA8 with tRNS), like the image crate's expand
        img.ch = trns.empty() ? 3 : 4; img.px.resize((size_t)w * h * img.ch);
        for (uint32_t y = 0; y < h; ++y) for (uint32_t x = 0; x < w; ++x) {
            const unsigned k = sample(y, x); uint8_t *q = &img.px[((size_t)y * w + x) * img.ch];
            for (int c = 0; c < 3; ++c) q[c] = 3 * k + c < plte.size() ? plte[3 * k + c] : 0;
            if (img.ch == 4) q[3] = k < trns.size() ? trns[k] : 255;
        }
        img.supported = true;
        return true;
    }
    img.ch = nch; img.px.resize((size_t)w * h * nch);
    for (uint32_t y = 0; y < h; ++y) for (size_t k = 0; k < (size_t)w * nch; ++k) img.px[(size_t)y * w * nch + k] = (uint8_t)sample(y, k);
    img.supported = (nch == 3 || nch == 4) && depth == 8; // R8, R8G8 and 16-bit formats: "unsupported image format" (gltf.rs:91-97)
    return true;
}

// ---- baseline JPEG decoder (sequential DCT, Huffman, 8 bit; 1 or 3 components; restart intervals) ---------------------
// The reference decodes JPEG through image 0.23 / jpeg-decoder; IDCT rounding and chroma upsampling differ between
// decoders by a level or so, so JPEG textures are close to, not bit-identical with, any other host's (parity unpinned).
// Here: separable binary64 IDCT, libjpeg-style triangle chroma upsampling (2x1, 2x2), JFIF YCbCr -> RGB.  Progressive
// files are refused.
struct JpegDec {
    const uint8_t *p; size_t n, pos = 0; std::string err;
    uint8_t qt[4][64]{}; bool have_qt[4]{};
    struct Huff { uint8_t bits[17]{}; uint8_t vals[256]{}; int mincode[17]{}, maxcode[18]{}, valptr[17]{}; bool ok = false; } dc[4], ac[4];
    struct Comp { int id = 0, h = 1, v = 1, tq = 0, td = 0, ta = 0, pred = 0; std::vector<uint8_t> plane; int pw = 0, ph = 0; } comp[3];
    int ncomp = 0, W = 0, H = 0, hmax = 1, vmax = 1, restart = 0;
    uint32_t bitbuf = 0; int bitcnt = 0; bool hit_marker = false;
    JpegDec(const std::string &d) : p((const uint8_t *)d.data()), n(d.size()) {}
    bool fail(const char *m) { if (err.empty()) err = m; return false; }
    int u8() { return pos < n ? p[pos++] : 0; }
    int u16() { int a = u8(); return (a << 8) | u8(); }
    void build(Huff &h) {
        int code = 0, k = 0;
        for (int l = 1; l <= 16; ++l) { h.valptr[l] = k; h.mincode[l] = code; code += h.bits[l]; k += h.bits[l]; h.maxcode[l] = h.bits[l] ? code - 1 : -1; code <<= 1; }
        h.maxcode[17] = 0x7fffffff; h.ok = true;
    }
    int bit() {
        if (bitcnt == 0) {
            int b = 0;
            if (!hit_marker && pos < n) { b = p[pos++]; if (b == 0xFF) { int b2 = pos < n ? p[pos] : 0; if (b2 == 0) ++pos; else { hit_marker = true; --pos; b = 0; } } }
            bitbuf = (uint32_t)b; bitcnt = 8;
        }
        --bitcnt; return (int)((bitbuf >> bitcnt) & 1u);
    }
    int bits(int k) { int v = 0; while (k-- > 0) v = (v << 1) | bit(); return v; }
    int decode(const Huff &h) {
        int code = 0;
        for (int l = 1; l <= 16; ++l) { code = (code << 1) | bit(); if (h.maxcode[l] >= 0 && code <= h.maxcode[l] && code >= h.mincode[l]) return h.vals[h.valptr[l] + code - h.mincode[l]]; }
        return -1;
    }
    static int extend(int v, int t) { return t == 0 ? 0 : (v < (1 << (t - 1)) ? v - (1 << t) + 1 : v); }
    bool block(Comp &c, int bx, int by) {
        static const uint8_t zz[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
        double coef[64] = {0};
        int t = decode(dc[c.td]); if (t < 0 || t > 11) return fail("bad JPEG DC code");
        c.pred += extend(bits(t), t);
        coef[0] = (double)c.pred * qt[c.tq][0];
        for (int k = 1; k < 64;) {
            const int rs = decode(ac[c.ta]); if (rs < 0) return fail("bad JPEG AC code");
            const int r = rs >> 4, sz = rs & 15;
            if (sz == 0) { if (r == 15) { k += 16; continue; } break; }
            k += r; if (k > 63) return fail("JPEG coefficient overrun");
            coef[zz[k]] = (double)extend(bits(sz), sz) * qt[c.tq][k]; ++k;
        }
        static double cs[8][8]; static bool init = false;
        if (!init) { for (int x = 0; x < 8; ++x) for (int u = 0; u < 8; ++u) cs[x][u] = (u == 0 ? std::sqrt(0.125) : 0.5) * std::cos((2 * x + 1) * u * 3.14159265358979323846 / 16.0); init = true; }
        double tmp[64];
        for (int v = 0; v < 8; ++v) for (int x = 0; x < 8; ++x) { double a = 0; for (int u = 0; u < 8; ++u) a += cs[x][u] * coef[8 * v + u]; tmp[8 * v + x] = a; }
        for (int y = 0; y < 8; ++y) for (int x = 0; x < 8; ++x) {
            double a = 0; for (int v = 0; v < 8; ++v) a += cs[y][v] * tmp[8 * v + x];
            const int px = 8 * bx + x, py = 8 * by + y;
            if (px < c.pw && py < c.ph) { double q = std::floor(a + 128.5); c.plane[(size_t)py * c.pw + px] = (uint8_t)(q < 0 ? 0 : (q > 255 ? 255 : q)); }
        }
        return true;
    }
    bool run(Image8 &img) {
        if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return fail("not a JPEG file");
        pos = 2;
        for (;;) {
            if (pos + 4 > n) return fail("truncated JPEG");
            if (u8() != 0xFF) return fail("JPEG marker expected");
            int m = u8(); while (m == 0xFF) m = u8();
            if (m == 0xD9) return fail("JPEG without image data");
            const size_t seg = pos; const int len = u16();
            if (len < 2 || seg + len > n) return fail("bad JPEG segment length");
            if (m == 0xDB) { while (pos < seg + len) { const int pq = u8(); if (pq >> 4) return fail("16-bit JPEG quantisation tables are not supported"); for (int k = 0; k < 64; ++k) qt[pq & 3][k] = (uint8_t)u8(); have_qt[pq & 3] = true; } }
            else if (m == 0xC4) { while (pos < seg + len) { const int th = u8(); Huff &h = (th >> 4) ? ac[th & 3] : dc[th & 3]; int tot = 0; for (int l = 1; l <= 16; ++l) { h.bits[l] = (uint8_t)u8(); tot += h.bits[l]; } if (tot > 256) return fail("bad JPEG Huffman table"); for (int k = 0; k < tot; ++k) h.vals[k] = (uint8_t)u8(); build(h); } }
            else if (m == 0xC0 || m == 0xC1) {
                if (u8() != 8) return fail("only 8-bit JPEG is supported");
                H = u16(); W = u16(); ncomp = u8();
                if ((ncomp != 1 && ncomp != 3) || W <= 0 || H <= 0) return fail("unsupported JPEG component count");
                for (int i = 0; i < ncomp; ++i) { comp[i].id = u8(); const int hv = u8(); comp[i].h = hv >> 4; comp[i].v = hv & 15; comp[i].tq = u8() & 3; if (comp[i].h < 1 || comp[i].h > 2 || comp[i].v < 1 || comp[i].v > 2) return fail("unsupported JPEG sampling factors"); hmax = std::max(hmax, comp[i].h); vmax = std::max(vmax, comp[i].v); }
            } else if (m == 0xC2 || (m >= 0xC5 && m <= 0xCF && m != 0xC8 && m != 0xCC)) return fail("progressive / arithmetic JPEG is not supported by the C++ host");
            else if (m == 0xDD) restart = u16();
            else if (m == 0xDA) {
                if (!W) return fail("JPEG scan before frame header");
                const int ns = u8(); if (ns != ncomp) return fail("non-interleaved JPEG scans are not supported");
                for (int i = 0; i < ns; ++i) { const int id = u8(), t = u8(); for (int j = 0; j < ncomp; ++j) if (comp[j].id == id) { comp[j].td = t >> 4; comp[j].ta = t & 15; } }
                pos = seg + len;
                const int mcuw = 8 * hmax, mcuh = 8 * vmax, mx = (W + mcuw - 1) / mcuw, my = (H + mcuh - 1) / mcuh;
                for (int i = 0; i < ncomp; ++i) { Comp &c = comp[i]; c.pw = mx * 8 * c.h; c.ph = my * 8 * c.v; c.plane.assign((size_t)c.pw * c.ph, 0); if (!have_qt[c.tq] || !dc[c.td].ok || !ac[c.ta].ok) return fail("JPEG table missing"); }
                int todo = restart;
                for (int yy = 0; yy < my; ++yy) for (int xx = 0; xx < mx; ++xx) {
                    if (restart && todo == 0) { // RSTn: byte-align, skip the marker, reset predictors
                        bitcnt = 0; hit_marker = false;
                        while (pos + 1 < n && !(p[pos] == 0xFF && p[pos + 1] >= 0xD0 && p[pos + 1] <= 0xD7)) ++pos;
                        pos += 2; for (int i = 0; i < ncomp; ++i) comp[i].pred = 0; todo = restart;
                    }
                    for (int i = 0; i < ncomp; ++i) for (int by = 0; by < comp[i].v; ++by) for (int bx = 0; bx < comp[i].h; ++bx) if (!block(comp[i], xx * comp[i].h + bx, yy * comp[i].v + by)) return false;
                    if (restart) --todo;
                }
                break;
            }
            pos = seg + len;
        }
        img.w = W; img.h = H; img.ch = ncomp == 1 ? 1 : 3; img.px.resize((size_t)W * H * img.ch);
        // chroma planes to full resolution: libjpeg's "fancy" (triangle) upsampling for 2x1 and 2x2, as jpeg-decoder does
        std::vector<uint8_t> full[3];
        for (int i = 0; i < ncomp; ++i) {
            const Comp &k = comp[i];
            const int fw = k.pw * hmax / k.h, fh = k.ph * vmax / k.v;
            full[i].resize((size_t)fw * fh);
            auto at = [&](int x, int y) -> int { x = x < 0 ? 0 : (x >= k.pw ? k.pw - 1 : x); y = y < 0 ? 0 : (y >= k.ph ? k.ph - 1 : y); return k.plane[(size_t)y * k.pw + x]; };
            const int fx = hmax / k.h, fy = vmax / k.v;
            for (int y = 0; y < fh; ++y) for (int x = 0; x < fw; ++x) {
                int v;
                if (fx == 1 && fy == 1) v = at(x, y);
                else if (fx == 2 && fy == 1) { const int c = x >> 1; v = (x & 1) ? (3 * at(c, y) + at(c + 1, y) + 2) >> 2 : (3 * at(c, y) + at(c - 1, y) + 1) >> 2; }
                else if (fx == 2 && fy == 2) {
                    const int c = x >> 1, r = y >> 1, r2 = (y & 1) ? r + 1 : r - 1;
                    const int cur = 3 * at(c, r) + at(c, r2), side = (x & 1) ? 3 * at(c + 1, r) + at(c + 1, r2) : 3 * at(c - 1, r) + at(c - 1, r2);
                    v = (3 * cur + side + ((x & 1) ? 7 : 8)) >> 4;
                } else v = at(x / fx, y / fy); // 1x2 and anything else: replicate
                full[i][(size_t)y * fw + x] = (uint8_t)v;
            }
        }
        const int fw0 = comp[0].pw * hmax / comp[0].h;
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
            if (ncomp == 1) { img.px[(size_t)y * W + x] = full[0][(size_t)y * fw0 + x]; continue; }
            double c[3];
            for (int i = 0; i < 3; ++i) c[i] = full[i][(size_t)y * (comp[i].pw * hmax / comp[i].h) + x];
            const double r = c[0] + 1.402 * (c[2] - 128.0), g = c[0] - 0.344136 * (c[1] - 128.0) - 0.714136 * (c[2] - 128.0), b = c[0] + 1.772 * (c[1] - 128.0);
            const double v3[3] = {r, g, b};
            for (int i = 0; i < 3; ++i) { double q = std::floor(v3[i] + 0.5); img.px[((size_t)y * W + x) * 3 + i] = (uint8_t)(q < 0 ? 0 : (q > 255 ? 255 : q)); }
        }
        img.supported = img.ch == 3; // greyscale = L8: "unsupported image format" for the importer (gltf.rs:91-97)
        return true;
    }
};
bool decode_image(const std::string &d, Image8 &img, std::string &err) {
    if (d.size() > 2 && (unsigned char)d[0] == 0xFF && (unsigned char)d[1] == 0xD8) { JpegDec j(d); if (!j.run(img)) { err = j.err; return false; } return true; }
    return decode_png(d, img, err);
}

// ---- MIP pyramid (texture.rs:213-236,279-405; same order as textures.py:build_mipmap) ---------------------------
float lanczos(float x, float tau = 2.0f) {
    x = std::fabs(x);
    if (x < 1e-5f) return 1.0f;
    if (x > 1.0f) return 0.0f;
    x = x * 3.14159274101257324f;
    const float s = (float)std::sin((double)(x * tau)) / (x * tau);
    return s * ((float)std::sin((double)x) / x);
}
struct RW { long first; float w[4]; };
std::vector<RW> resample_weights(int old_res, int new_res) {
    std::vector<RW> out((size_t)new_res);
    for (int i = 0; i < new_res; ++i) {
        const float center = ((float)i + 0.5f) * (float)old_res / (float)new_res;
        const float first = std::floor((center - 2.0f) + 0.5f);
        RW r;
        for (int j = 0; j < 4; ++j) r.w[j] = lanczos((first + (float)j + 0.5f - center) / 2.0f);
        const float inv = 1.0f / (((r.w[0] + r.w[1]) + r.w[2]) + r.w[3]);
        for (int j = 0; j < 4; ++j) r.w[j] = r.w[j] * inv;
        r.first = std::max((long)first, 0L); // `first_texel as usize` saturates at 0
        out[(size_t)i] = r;
    }
    return out;
}
long wrap_index(long i, long n, int wrap) {
    if (wrap == PTRS_WRAP_REPEAT) { long m = i % n; return m < 0 ? m + n : m; }
    if (wrap == PTRS_WRAP_CLAMP) return std::min(std::max(i, 0L), n - 1);
    return i;
}
int round_up_pow2i(int v) { int p = 1; while (p < v) p <<= 1; return p; }
TexImage *build_mipmap(RenderScene &s, std::vector<float> img, int rows, int cols, int ch, int wrap) {
    if ((cols & (cols - 1)) || (rows & (rows - 1))) {
        const int pc = round_up_pow2i(cols), pr = round_up_pow2i(rows);
        std::vector<float> res((size_t)pr * pc * ch, 0.0f);
        const auto sw = resample_weights(cols, pc);
        for (int t = 0; t < rows; ++t) for (int x = 0; x < pc; ++x) for (int j = 0; j < 4; ++j) {
            const long o = wrap_index(sw[(size_t)x].first + j, cols, wrap);
            if (0 < o && o < cols) for (int c = 0; c < ch; ++c) res[((size_t)t * pc + x) * ch + c] += img[((size_t)t * cols + o) * ch + c] * sw[(size_t)x].w[j]; // sic: texel 0 skipped (texture.rs:321)
        }
        const auto tw = resample_weights(rows, pr);
        std::vector<float> work((size_t)pr * ch);
        for (int x = 0; x < pc; ++x) {
            std::fill(work.begin(), work.end(), 0.0f);
            for (int t = 0; t < pr; ++t) for (int j = 0; j < 4; ++j) {
                const long o = wrap_index(tw[(size_t)t].first + j, rows, wrap);
                if (o < rows) for (int c = 0; c < ch; ++c) work[(size_t)t * ch + c] += res[((size_t)o * pc + x) * ch + c] * tw[(size_t)t].w[j];
            }
            for (int t = 0; t < pr; ++t) for (int c = 0; c < ch; ++c) res[((size_t)t * pc + x) * ch + c] = work[(size_t)t * ch + c];
        }
        img.swap(res); rows = pr; cols = pc;
    }
    auto ti = std::make_unique<TexImage>();
    ti->channels = ch;
    ti->levels.push_back(std::move(img)); ti->rows.push_back(rows); ti->cols.push_back(cols);
    int n_levels = 1; for (int m = std::max(rows, cols); m > 1; m >>= 1) ++n_levels;
    for (int l = 1; l < n_levels; ++l) {
        const std::vector<float> &prev = ti->levels.back();
        const int pr = ti->rows.back(), pc = ti->cols.back(), tr = std::max(1, pr / 2), sr = std::max(1, pc / 2);
        std::vector<float> nxt((size_t)tr * sr * ch);
        auto tex = [&](long si, long tj, int c) -> float {
            if (wrap == PTRS_WRAP_BLACK) { if (si >= pc || tj >= pr) return 0.0f; }
            else { si = wrap_index(si, pc, wrap); tj = wrap_index(tj, pr, wrap); }
            return prev[((size_t)tj * pc + si) * ch + c];
        };
        for (int t = 0; t < tr; ++t) for (int x = 0; x < sr; ++x) for (int c = 0; c < ch; ++c)
            nxt[((size_t)t * sr + x) * ch + c] = (((tex(2 * x, 2 * t, c) + tex(2 * x + 1, 2 * t, c)) + tex(2 * x, 2 * t + 1, c)) + tex(2 * x + 1, 2 * t + 1, c)) * 0.25f;
        ti->levels.push_back(std::move(nxt)); ti->rows.push_back(tr); ti->cols.push_back(sr);
    }
    for (auto &lv : ti->levels) ti->ptrs.push_back(lv.data());
    s.images.push_back(std::move(ti));
    return s.images.back().get();
}
int32_t add_image_texture(RenderScene &s, std::vector<float> texels, int rows, int cols, int ch, int wrap) {
    TexImage *ti = build_mipmap(s, std::move(texels), rows, cols, ch, wrap);
    PtrsTexture t{}; t.kind = PTRS_TEX_IMAGE; t.channels = ch; t.su = t.sv = 1.0f; t.du = t.dv = 0.0f; t.wrap = wrap;
    t.n_levels = (int32_t)ti->levels.size(); t.level_data = ti->ptrs.data(); t.level_cols = ti->cols.data(); t.level_rows = ti->rows.data();
    s.textures.push_back(t);
    return (int32_t)s.textures.size() - 1;
}
float inverse_gamma_correct(float v) { // common/math.rs:141-147
    if (v <= 0.04045f) return v * 1.0f / 12.92f;
    return (float)std::pow((double)((v + 0.055f) * 1.0f / 1.055f), 2.4);
}
int32_t const_tex(RenderScene &s, int ch, float a, float b = 0.0f, float c = 0.0f) {
    PtrsTexture t{}; t.kind = PTRS_TEX_CONSTANT; t.channels = ch; t.value[0] = a; t.value[1] = b; t.value[2] = c; t.su = t.sv = 1.0f;
    s.textures.push_back(t);
    return (int32_t)s.textures.size() - 1;
}
int32_t add_mat(RenderScene &s, int kind, std::initializer_list<int32_t> tex, int32_t inner = -1) {
    PtrsMaterial m{}; m.kind = kind; m.flags = 0; m.inner = inner;
    for (int k = 0; k < 6; ++k) m.tex[k] = -1;
    int k = 0; for (int32_t t : tex) m.tex[k++] = t;
    s.materials.push_back(m);
    return (int32_t)s.materials.size() - 1;
}

// ---- matrices -----------------------------------------------------------------------------------------------
struct M4 { float m[16]; }; // row-major
M4 ident() { M4 r{}; r.m[0] = r.m[5] = r.m[10] = r.m[15] = 1.0f; return r; }
M4 mul(const M4 &a, const M4 &b) {
    M4 r;
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { float acc = a.m[4 * i] * b.m[j]; for (int k = 1; k < 4; ++k) acc = acc + a.m[4 * i + k] * b.m[4 * k + j]; r.m[4 * i + j] = acc; }
    return r;
}
M4 quat_to_mat4(const float q[4]) { // UnitQuaternion::to_homogeneous
    const float i = q[0], j = q[1], k = q[2], w = q[3];
    const float ww = w * w, ii = i * i, jj = j * j, kk = k * k;
    const float ij = i * j * 2.0f, wk = w * k * 2.0f, wj = w * j * 2.0f, ik = i * k * 2.0f, jk = j * k * 2.0f, wi = w * i * 2.0f;
    M4 r = ident();
    r.m[0] = ww + ii - jj - kk; r.m[1] = ij - wk; r.m[2] = wj + ik;
    r.m[4] = wk + ij; r.m[5] = ww - ii + jj - kk; r.m[6] = jk - wi;
    r.m[8] = ik - wj; r.m[9] = wi + jk; r.m[10] = ww - ii - jj + kk;
    return r;
}
void floats_of(const JVal *v, float *out, size_t n) { if (v && v->type == JVal::Arr) for (size_t k = 0; k < n && k < v->a.size(); ++k) out[k] = (float)v->a[k].n; }
M4 node_transform(const JVal &node) { // trans_from_gltf (common/importer/gltf.rs:87-96); a `matrix` node is used as given
    if (const JVal *mv = node.get("matrix")) { float c[16] = {0}; floats_of(mv, c, 16); M4 r; for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) r.m[4 * i + j] = c[4 * j + i]; return r; }
    float t[3] = {0, 0, 0}, q[4] = {0, 0, 0, 1}, sc[3] = {1, 1, 1};
    floats_of(node.get("translation"), t, 3); floats_of(node.get("rotation"), q, 4); floats_of(node.get("scale"), sc, 3);
    M4 T = ident(); T.m[3] = t[0]; T.m[7] = t[1]; T.m[11] = t[2];
    M4 S = ident(); S.m[0] = sc[0]; S.m[5] = sc[1]; S.m[10] = sc[2];
    return mul(mul(T, quat_to_mat4(q)), S);
}
void xf_point(const M4 &m, const float *p, float *o) {
    for (int r = 0; r < 3; ++r) o[r] = ((m.m[4 * r] * p[0] + m.m[4 * r + 1] * p[1]) + m.m[4 * r + 2] * p[2]) + m.m[4 * r + 3];
    if (!(m.m[12] == 0.0f && m.m[13] == 0.0f && m.m[14] == 0.0f && m.m[15] == 1.0f)) { const float w = ((m.m[12] * p[0] + m.m[13] * p[1]) + m.m[14] * p[2]) + m.m[15]; for (int r = 0; r < 3; ++r) o[r] = o[r] / w; }
}
void xf_vector(const M4 &m, const float *v, float *o) { for (int r = 0; r < 3; ++r) o[r] = (m.m[4 * r] * v[0] + m.m[4 * r + 1] * v[1]) + m.m[4 * r + 2] * v[2]; }
void quat_from_rotation(const float r[3][3], float q[4]) { // UnitQuaternion::from_rotation_matrix -> (i, j, k, w)
    const float tr = (r[0][0] + r[1][1]) + r[2][2], qq = 0.25f; float w, i, j, k;
    if (tr > 0.0f) { float d = std::sqrt(tr + 1.0f) * 2.0f; w = qq * d; i = (r[2][1] - r[1][2]) / d; j = (r[0][2] - r[2][0]) / d; k = (r[1][0] - r[0][1]) / d; }
    else if (r[0][0] > r[1][1] && r[0][0] > r[2][2]) { float d = std::sqrt(((1.0f + r[0][0]) - r[1][1]) - r[2][2]) * 2.0f; w = (r[2][1] - r[1][2]) / d; i = qq * d; j = (r[0][1] + r[1][0]) / d; k = (r[0][2] + r[2][0]) / d; }
    else if (r[1][1] > r[2][2]) { float d = std::sqrt(((1.0f + r[1][1]) - r[0][0]) - r[2][2]) * 2.0f; w = (r[0][2] - r[2][0]) / d; i = (r[0][1] + r[1][0]) / d; j = qq * d; k = (r[1][2] + r[2][1]) / d; }
    else { float d = std::sqrt(((1.0f + r[2][2]) - r[0][0]) - r[1][1]) * 2.0f; w = (r[1][0] - r[0][1]) / d; i = (r[0][2] + r[2][0]) / d; j = (r[1][2] + r[2][1]) / d; k = qq * d; }
    q[0] = i; q[1] = j; q[2] = k; q[3] = w;
}

// ---- the importer -------------------------------------------------------------------------------------------
struct Importer {
    JVal doc; std::vector<std::string> buffers; std::string base, err;
    RenderScene *scene = nullptr;
    std::map<int, Image8> images;
    std::vector<int32_t> materials;
    std::vector<PtrsLight> deferred; // directional lights join the list after the traversal (gltf.rs:567-575)
    bool fail(const std::string &m) { if (err.empty()) err = m; return false; }

    bool load(const std::string &path) {
        std::string raw;
        if (!read_file(path, raw)) return fail("cannot open " + path);
        base = dir_of(path);
        std::string glb_bin; bool have_bin = false, is_glb = raw.size() >= 12 && raw.compare(0, 4, "glTF") == 0;
        std::string json = raw;
        if (is_glb) {
            uint32_t ver, len; std::memcpy(&ver, raw.data() + 4, 4); std::memcpy(&len, raw.data() + 8, 4);
            if (ver != 2) return fail("unsupported GLB version");
            size_t off = 12; json.clear();
            while (off + 8 <= std::min<size_t>(len, raw.size())) {
                uint32_t cl, ct; std::memcpy(&cl, raw.data() + off, 4); std::memcpy(&ct, raw.data() + off + 4, 4);
                if (off + 8 + cl > raw.size()) return fail("truncated GLB chunk");
                if (ct == 0x4E4F534Au) json = raw.substr(off + 8, cl);
                else if (ct == 0x004E4942u && !have_bin) { glb_bin = raw.substr(off + 8, cl); have_bin = true; }
                off += 8 + cl + ((4 - cl % 4) % 4);
            }
            if (json.empty()) return fail("GLB without a JSON chunk");
        }
        JParser P(json);
        if (!P.value(doc)) return fail("JSON: " + P.err);
        if (const JVal *bs = doc.get("buffers")) for (size_t i = 0; i < bs->size(); ++i) {
            const JVal &b = bs->at(i); std::string data;
            if (!b.has("uri")) { if (!have_bin) return fail("buffer without uri and no BIN chunk"); data = glb_bin; }
            else { const std::string uri = b.str("uri"); if (uri.compare(0, 5, "data:") == 0) data = base64_decode(uri.substr(uri.find(',') + 1)); else if (!read_file(base + "/" + uri, data)) return fail("cannot open " + base + "/" + uri); }
            if (data.size() < (size_t)b.num("byteLength", 0)) return fail("buffer shorter than its byteLength");
            buffers.push_back(std::move(data));
        }
        return true;
    }

    // accessor -> doubles (count * ncomp) + component type
    bool accessor(int index, std::vector<double> &out, int &ncomp, int &ctype) {
        const JVal *accs = doc.get("accessors");
        if (!accs || index < 0 || (size_t)index >= accs->size()) return fail("accessor index out of range");
        const JVal &a = accs->at((size_t)index);
        if (a.has("sparse")) return fail("sparse accessors are not supported");
        ctype = a.integer("componentType", 0);
        const std::string ty = a.str("type");
        ncomp = ty == "SCALAR" ? 1 : ty == "VEC2" ? 2 : ty == "VEC3" ? 3 : ty == "VEC4" ? 4 : ty == "MAT4" ? 16 : ty == "MAT3" ? 9 : ty == "MAT2" ? 4 : 0;
        const size_t csz = ctype == 5120 || ctype == 5121 ? 1 : ctype == 5122 || ctype == 5123 ? 2 : ctype == 5125 || ctype == 5126 ? 4 : 0;
        if (!ncomp || !csz) return fail("unsupported accessor type");
        const size_t count = (size_t)a.num("count", 0);
        out.assign(count * ncomp, 0.0);
        if (!a.has("bufferView")) return true;
        const JVal *bvs = doc.get("bufferViews"); const int bvi = a.integer("bufferView", -1);
        if (!bvs || bvi < 0 || (size_t)bvi >= bvs->size()) return fail("bufferView index out of range");
        const JVal &bv = bvs->at((size_t)bvi);
        const int bi = bv.integer("buffer", -1);
        if (bi < 0 || (size_t)bi >= buffers.size()) return fail("buffer index out of range");
        const std::string &data = buffers[(size_t)bi];
        const size_t start = (size_t)bv.num("byteOffset", 0) + (size_t)a.num("byteOffset", 0), elem = csz * ncomp;
        size_t stride = (size_t)bv.num("byteStride", 0); if (!stride) stride = elem;
        if (count && start + stride * (count - 1) + elem > data.size()) return fail("accessor " + std::to_string(index) + " reaches past its buffer");
        for (size_t i = 0; i < count; ++i) for (int c = 0; c < ncomp; ++c) {
            const char *p = data.data() + start + stride * i + csz * c;
            double v = 0;
            switch (ctype) {
                case 5120: { int8_t x; std::memcpy(&x, p, 1); v = x; break; } case 5121: { uint8_t x; std::memcpy(&x, p, 1); v = x; break; }
                case 5122: { int16_t x; std::memcpy(&x, p, 2); v = x; break; } case 5123: { uint16_t x; std::memcpy(&x, p, 2); v = x; break; }
                case 5125: { uint32_t x; std::memcpy(&x, p, 4); v = x; break; } default: { float x; std::memcpy(&x, p, 4); v = x; }
            }
            out[i * ncomp + c] = v;
        }
        return true;
    }

    const Image8 *image(const JVal &tex_info) {
        const JVal *texs = doc.get("textures"); const int ti = tex_info.integer("index", -1);
        if (!texs || ti < 0 || (size_t)ti >= texs->size()) { fail("texture index out of range"); return nullptr; }
        const int src = texs->at((size_t)ti).integer("source", -1);
        auto it = images.find(src);
        if (it != images.end()) return &it->second;
        const JVal *imgs = doc.get("images");
        if (!imgs || src < 0 || (size_t)src >= imgs->size()) { fail("image index out of range"); return nullptr; }
        const JVal &im = imgs->at((size_t)src); std::string data;
        if (im.has("uri")) { const std::string uri = im.str("uri"); if (uri.compare(0, 5, "data:") == 0) data = base64_decode(uri.substr(uri.find(',') + 1)); else if (!read_file(base + "/" + uri, data)) { fail("cannot open " + base + "/" + uri); return nullptr; } }
        else {
            const JVal *bvs = doc.get("bufferViews"); const int bvi = im.integer("bufferView", -1);
            if (!bvs || bvi < 0 || (size_t)bvi >= bvs->size()) { fail("image bufferView out of range"); return nullptr; }
            const JVal &bv = bvs->at((size_t)bvi); const int bi = bv.integer("buffer", -1);
            if (bi < 0 || (size_t)bi >= buffers.size()) { fail("buffer index out of range"); return nullptr; }
            const size_t o = (size_t)bv.num("byteOffset", 0), n = (size_t)bv.num("byteLength", 0);
            if (o + n > buffers[(size_t)bi].size()) { fail("image reaches past its buffer"); return nullptr; }
            data = buffers[(size_t)bi].substr(o, n);
        }
        Image8 img;
        if (!decode_image(data, img, err)) return nullptr;
        return &(images[src] = std::move(img));
    }
    bool wrap_mode(const JVal &tex_info, int &wrap) { // wrap_mode_from_gtlf (gltf.rs:30-36) + the wrapS == wrapT asserts
        const JVal &t = doc.get("textures")->at((size_t)tex_info.integer("index", 0));
        int ws = 10497, wt = 10497;
        if (t.has("sampler")) { const JVal *ss = doc.get("samplers"); const int si = t.integer("sampler", -1); if (!ss || si < 0 || (size_t)si >= ss->size()) return fail("sampler index out of range"); ws = ss->at((size_t)si).integer("wrapS", 10497); wt = ss->at((size_t)si).integer("wrapT", 10497); }
        if (ws != wt) return fail("sampler with wrapS != wrapT (the reference asserts)");
        wrap = ws == 33071 ? PTRS_WRAP_CLAMP : PTRS_WRAP_REPEAT;
        return true;
    }
    // color_texture_from_gltf (gltf.rs:38-98): RGB (alpha dropped), gamma-decoded, scaled by factor; -1 = "None"
    bool color_texture(const JVal &info, const float factor[3], int32_t &out) {
        out = -1;
        const Image8 *img = image(info);
        if (!img) return false;
        if (!img->supported) return true;
        int wrap; if (!wrap_mode(info, wrap)) return false;
        std::vector<float> v((size_t)img->w * img->h * 3);
        for (size_t p = 0; p < (size_t)img->w * img->h; ++p) for (int c = 0; c < 3; ++c) v[3 * p + c] = factor[c] * inverse_gamma_correct((float)img->px[p * img->ch + c] / 255.0f);
        out = add_image_texture(*scene, std::move(v), img->h, img->w, 3, wrap);
        return true;
    }
    bool float_texture(const Image8 &img, int channel, float scale, int wrap, int32_t &out) { // ImageTexture::<f32>::new (texture.rs:97-121)
        std::vector<float> v((size_t)img.w * img.h);
        for (size_t p = 0; p < v.size(); ++p) v[p] = scale * ((float)img.px[p * img.ch + channel] / 255.0f);
        out = add_image_texture(*scene, std::move(v), img.h, img.w, 1, wrap);
        return true;
    }

    bool material(const JVal &m, int32_t &out) { // material_from_gltf (gltf.rs:170-296)
        RenderScene &s = *scene;
        static const JVal empty_obj = [] { JVal v; v.type = JVal::Obj; return v; }();
        const JVal &pbr = m.get("pbrMetallicRoughness") ? *m.get("pbrMetallicRoughness") : empty_obj;
        float bcf[4] = {1, 1, 1, 1}; floats_of(pbr.get("baseColorFactor"), bcf, 4);
        const float cf[3] = {inverse_gamma_correct(bcf[0]), inverse_gamma_correct(bcf[1]), inverse_gamma_correct(bcf[2])};
        int32_t color_tex = -1;
        if (const JVal *t = pbr.get("baseColorTexture")) if (!color_texture(*t, cf, color_tex)) return false;
        if (color_tex < 0) color_tex = const_tex(s, 3, cf[0], cf[1], cf[2]);
        int32_t normal_tex = -1;
        if (const JVal *info = m.get("normalTexture")) {
            const Image8 *img = image(*info);
            if (!img) return false;
            if (!img->supported) return fail("normal texture with an unsupported image format (the reference unwraps)");
            int wrap; if (!wrap_mode(*info, wrap)) return false;
            const float sc = (float)info->num("scale", 1.0);
            std::vector<float> v((size_t)img->w * img->h * 3); // RgbImage::from_raw on the raw stream
            for (size_t k = 0; k < v.size(); ++k) { float x = (float)img->px[k] / 127.5f - 1.0f; if (k % 3 != 2) x *= sc; v[k] = x; }
            normal_tex = add_image_texture(s, std::move(v), img->h, img->w, 3, wrap);
        }
        auto with_normal = [&](int32_t mat) { return normal_tex >= 0 ? add_mat(s, PTRS_MAT_NORMAL, {normal_tex}, mat) : mat; };
        const JVal *ext = m.get("extensions");
        float transmission = 0.0f, ior = 1.5f;
        if (ext) { if (const JVal *t = ext->get("KHR_materials_transmission")) transmission = (float)t->num("transmissionFactor", 0.0); if (const JVal *t = ext->get("KHR_materials_ior")) ior = (float)t->num("ior", 1.5); }
        if (transmission == 1.0f) { const int32_t a = const_tex(s, 3, 1, 1, 1), b = const_tex(s, 3, 1, 1, 1), c = const_tex(s, 1, ior); out = with_normal(add_mat(s, PTRS_MAT_GLASS, {a, b, c})); return true; }
        const float alpha = bcf[3];
        if (m.str("alphaMode", "OPAQUE") == "BLEND" && alpha < 1.0f) {
            const int32_t a = const_tex(s, 3, 1, 1, 1), b = const_tex(s, 3, 1.0f - alpha * cf[0], 1.0f - alpha * cf[1], 1.0f - alpha * cf[2]), c = const_tex(s, 1, 1.33f);
            out = with_normal(add_mat(s, PTRS_MAT_GLASS, {a, b, c})); return true;
        }
        const float metallic = (float)pbr.num("metallicFactor", 1.0), roughness = (float)pbr.num("roughnessFactor", 1.0);
        if (metallic == 1.0f && roughness == 0.0f) { out = add_mat(s, PTRS_MAT_MIRROR, {}); return true; }
        int32_t mt = const_tex(s, 1, metallic), rt = const_tex(s, 1, roughness);
        if (const JVal *info = pbr.get("metallicRoughnessTexture")) { // metallic = B, roughness = G (gltf.rs:100-168)
            const Image8 *img = image(*info);
            if (!img) return false;
            if (img->supported) { int wrap; if (!wrap_mode(*info, wrap)) return false; float_texture(*img, 2, metallic, wrap, mt); float_texture(*img, 1, roughness, wrap, rt); }
        }
        const int32_t it = const_tex(s, 1, ior);
        out = with_normal(add_mat(s, PTRS_MAT_DISNEY, {color_tex, mt, it, rt}));
        return true;
    }

    // populate_scene's 10x10 probe (gltf.rs:413-427): ke at Triangle::sample((x/10, y/10)), level-0 bilinear
    static bool has_emission(const TexImage &ti, int wrap, const float uv[3][2]) {
        const int rows = ti.rows[0], cols = ti.cols[0], ch = ti.channels; const std::vector<float> &l0 = ti.levels[0];
        for (int x = 0; x < 10; ++x) for (int y = 0; y < 10; ++y) {
            const float u0 = (float)x * 0.1f, u1 = (float)y * 0.1f, su0 = std::sqrt(u0);
            const float b0 = 1.0f - su0, b1 = u1 * su0, b2 = (1.0f - b0) - b1;
            const float st0 = (b0 * uv[0][0] + b1 * uv[1][0]) + b2 * uv[2][0], st1 = (b0 * uv[0][1] + b1 * uv[1][1]) + b2 * uv[2][1];
            const long s0 = (long)std::floor(st0 * (float)cols - 0.5f), t0 = (long)std::floor(st1 * (float)rows - 0.5f);
            for (int ds = 0; ds < 2; ++ds) for (int dt = 0; dt < 2; ++dt) {
                long si = s0 + ds, tj = t0 + dt;
                if (wrap == PTRS_WRAP_BLACK) { if (si < 0 || si >= cols || tj < 0 || tj >= rows) continue; }
                else { si = wrap_index(si, cols, wrap); tj = wrap_index(tj, rows, wrap); }
                for (int c = 0; c < ch; ++c) if (l0[((size_t)tj * cols + si) * ch + c] != 0.0f) return true;
            }
        }
        return false;
    }

    bool primitive(const JVal &prim, const M4 &xf) { // shapes_from_gltf_prim + the emissive part of populate_scene
        RenderScene &s = *scene;
        if (prim.integer("mode", 4) != 4) return fail("only triangle-list primitives are supported (the reference unwraps read_indices on them)");
        if (!prim.has("indices")) return fail("primitive without indices (the reference unwraps)");
        static const JVal empty_obj = [] { JVal v; v.type = JVal::Obj; return v; }();
        const JVal *mats = doc.get("materials");
        const int mat_index = prim.integer("material", -1);
        if (mat_index >= 0 && (!mats || (size_t)mat_index >= mats->size())) return fail("material index out of range");
        const JVal &mat = mat_index >= 0 ? mats->at((size_t)mat_index) : empty_obj;
        Mesh mesh;
        const JVal *pbr = mat.get("pbrMetallicRoughness"), *bct = pbr ? pbr->get("baseColorTexture") : nullptr;
        if (bct && mat.str("alphaMode", "OPAQUE") == "MASK") {
            const Image8 *img = image(*bct);
            if (!img) return false;
            if (!img->supported || img->ch != 4) return fail("alpha-mask material whose base colour image is not RGBA8 (the reference asserts)");
            int wrap; if (!wrap_mode(*bct, wrap)) return false;
            float_texture(*img, 3, 1.0f, wrap, mesh.alpha_mask_tex);
        }
        const JVal *attr = prim.get("attributes");
        if (!attr || !attr->has("POSITION")) return fail("primitive without POSITION (the reference unwraps)");
        std::vector<double> v; int nc, ct;
        if (!accessor(prim.integer("indices", -1), v, nc, ct)) return false;
        const size_t ntri = v.size() / 3;
        mesh.indices.resize(ntri * 3); for (size_t k = 0; k < ntri * 3; ++k) mesh.indices[k] = (uint32_t)v[k];
        if (!accessor(attr->integer("POSITION", -1), v, nc, ct) || nc != 3) return fail(err.empty() ? "POSITION must be VEC3" : err);
        const size_t nv = v.size() / 3;
        mesh.pos.resize(nv * 3);
        for (size_t k = 0; k < nv; ++k) { const float p[3] = {(float)v[3 * k], (float)v[3 * k + 1], (float)v[3 * k + 2]}; xf_point(xf, p, &mesh.pos[3 * k]); }
        for (uint32_t ix : mesh.indices) if (ix >= nv) return fail("index out of range");
        if (attr->has("NORMAL")) { if (!accessor(attr->integer("NORMAL", -1), v, nc, ct) || nc != 3 || v.size() != nv * 3) return fail(err.empty() ? "NORMAL must be VEC3 per vertex" : err); mesh.normal.resize(nv * 3); for (size_t k = 0; k < nv; ++k) { const float p[3] = {(float)v[3 * k], (float)v[3 * k + 1], (float)v[3 * k + 2]}; xf_vector(xf, p, &mesh.normal[3 * k]); } }
        if (attr->has("TANGENT")) { if (!accessor(attr->integer("TANGENT", -1), v, nc, ct) || nc != 4 || v.size() != nv * 4) return fail(err.empty() ? "TANGENT must be VEC4 per vertex" : err); mesh.tangent.resize(nv * 3); for (size_t k = 0; k < nv; ++k) { const float p[3] = {(float)v[4 * k], (float)v[4 * k + 1], (float)v[4 * k + 2]}; xf_vector(xf, p, &mesh.tangent[3 * k]); } }
        if (attr->has("TEXCOORD_0")) {
            if (!accessor(attr->integer("TEXCOORD_0", -1), v, nc, ct) || nc != 2 || v.size() != nv * 2) return fail(err.empty() ? "TEXCOORD_0 must be VEC2 per vertex" : err);
            mesh.uv.resize(nv * 2);
            for (size_t k = 0; k < nv * 2; ++k) mesh.uv[k] = ct == 5126 ? (float)v[k] : ct == 5121 ? (float)v[k] / 255.0f : ct == 5123 ? (float)v[k] / 65535.0f : 0.0f; // into_f32()
            if (ct != 5126 && ct != 5121 && ct != 5123) return fail("unsupported normalised component type");
        }
        mesh.material = mat_index >= 0 ? materials[(size_t)mat_index + 1] : materials[0]; // default material on first idx
        const uint32_t mi = (uint32_t)s.meshes.size();
        float ef[3] = {0, 0, 0}; floats_of(mat.get("emissiveFactor"), ef, 3);
        const float e = 10.0f * ef[0]; // EMISSIVE_SCALING_FACTOR, red factor for all channels
        std::vector<float> uv_copy = mesh.uv; std::vector<uint32_t> idx_copy = mesh.indices;
        s.meshes.push_back(std::move(mesh));
        if (e == 0.0f) return true;
        int32_t ke = const_tex(s, 3, e, e, e); const TexImage *ke_img = nullptr; int ke_wrap = PTRS_WRAP_REPEAT;
        if (const JVal *et = mat.get("emissiveTexture")) {
            const float f3[3] = {e, e, e}; int32_t t;
            if (!color_texture(*et, f3, t)) return false;
            if (t >= 0) { ke = t; ke_img = s.images.back().get(); ke_wrap = s.textures[(size_t)t].wrap; }
        }
        for (uint32_t t = 0; t < ntri; ++t) {
            if (ke_img) {
                float uv[3][2] = {{0, 0}, {1, 0}, {1, 1}};
                if (!uv_copy.empty()) for (int k = 0; k < 3; ++k) { uv[k][0] = uv_copy[2 * idx_copy[3 * t + k]]; uv[k][1] = uv_copy[2 * idx_copy[3 * t + k] + 1]; }
                if (!has_emission(*ke_img, ke_wrap, uv)) continue;
            }
            PtrsLight L{}; L.kind = PTRS_LIGHT_AREA; L.mesh = mi; L.tri = t; L.ke_tex = ke; L.lmap_tex = -1;
            s.lights.push_back(L);
        }
        return true;
    }

    bool light(const JVal &l, const M4 &xf) { // populate_scene, KHR_lights_punctual part (gltf.rs:460-487)
        float col[3] = {1, 1, 1}; floats_of(l.get("color"), col, 3);
        const float c = (float)l.num("intensity", 1.0) * col[0];
        PtrsLight L{}; L.ke_tex = -1; L.lmap_tex = -1; L.c[0] = L.c[1] = L.c[2] = c;
        if (l.str("type") == "directional") {
            const float d[3] = {0, 0, -1}; float w[3]; xf_vector(xf, d, w);
            const float n = std::sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
            L.kind = PTRS_LIGHT_DIRECTIONAL; for (int k = 0; k < 3; ++k) L.v[k] = w[k] / n;
            deferred.push_back(L);
        } else { // point, and spot treated as point
            const float o[3] = {0, 0, 0}; L.kind = PTRS_LIGHT_POINT; xf_point(xf, o, L.v);
            scene->lights.push_back(L);
        }
        return true;
    }

    bool populate(const M4 &parent, int node_index, int depth = 0) {
        const JVal *nodes = doc.get("nodes");
        if (!nodes || node_index < 0 || (size_t)node_index >= nodes->size() || depth > 256) return fail("node index out of range");
        const JVal &node = nodes->at((size_t)node_index);
        const M4 xf = mul(parent, node_transform(node));
        if (node.has("mesh")) {
            const JVal *meshes = doc.get("meshes"); const int mi = node.integer("mesh", -1);
            if (!meshes || mi < 0 || (size_t)mi >= meshes->size()) return fail("mesh index out of range");
            if (const JVal *prims = meshes->at((size_t)mi).get("primitives")) for (size_t k = 0; k < prims->size(); ++k) if (!primitive(prims->at(k), xf)) return false;
        }
        if (const JVal *ext = node.get("extensions")) if (const JVal *lp = ext->get("KHR_lights_punctual")) if (lp->has("light")) {
            const JVal *dext = doc.get("extensions"), *dl = dext ? dext->get("KHR_lights_punctual") : nullptr, *ls = dl ? dl->get("lights") : nullptr;
            const int li = lp->integer("light", -1);
            if (!ls || li < 0 || (size_t)li >= ls->size()) return fail("light index out of range");
            if (!light(ls->at((size_t)li), xf)) return false;
        }
        if (const JVal *ch = node.get("children")) for (size_t k = 0; k < ch->size(); ++k) if (!populate(xf, (int)ch->at(k).n, depth + 1)) return false;
        return true;
    }

    // find_camera (common/importer/gltf.rs:3-46) incl. its first-child-only descent
    bool find_camera(const M4 &parent, int node_index, int rw, int rh, Camera &cam, int depth = 0) {
        const JVal *nodes = doc.get("nodes");
        if (!nodes || node_index < 0 || (size_t)node_index >= nodes->size() || depth > 256) return false;
        const JVal &node = nodes->at((size_t)node_index);
        const M4 xf = mul(parent, node_transform(node));
        if (node.has("camera")) {
            const JVal *cams = doc.get("cameras"); const int ci = node.integer("camera", -1);
            if (cams && ci >= 0 && (size_t)ci < cams->size() && cams->at((size_t)ci).str("type") == "perspective" && cams->at((size_t)ci).has("perspective")) {
                const JVal &p = *cams->at((size_t)ci).get("perspective");
                float r[3][3];
                for (int c = 0; c < 3; ++c) { const float x = xf.m[c], y = xf.m[4 + c], z = xf.m[8 + c], n = std::sqrt((x * x + y * y) + z * z); r[0][c] = x / n; r[1][c] = y / n; r[2][c] = z / n; }
                float q[4]; quat_from_rotation(r, q);
                const float tr[3] = {xf.m[3], xf.m[7], xf.m[11]};
                make_camera_perspective(q, tr, (float)rw / (float)rh, (float)p.num("yfov", 1.0), (float)p.num("znear", 0.01), (float)p.num("zfar", 10000.0), rw, rh, cam);
                return true;
            }
        }
        if (const JVal *ch = node.get("children")) if (ch->size() > 0) return find_camera(xf, (int)ch->at(0).n, rw, rh, cam, depth + 1);
        return false;
    }
};

// ---- Radiance RGBE + InfiniteAreaLight::new ------------------------------------------------------------------------
bool read_rgbe(const std::string &path, std::vector<float> &rgb, int &rows, int &cols, std::string &err) {
    std::string d;
    if (!read_file(path, d)) { err = "cannot open " + path; return false; }
    if (d.compare(0, 2, "#?") != 0) { err = "not a Radiance file"; return false; }
    size_t pos = 0;
    for (;;) { size_t e = d.find('\n', pos); if (e == std::string::npos) { err = "truncated Radiance header"; return false; } const bool blank = e == pos; pos = e + 1; if (blank) break; }
    size_t e = d.find('\n', pos); if (e == std::string::npos) { err = "truncated Radiance header"; return false; }
    char a[8], b[8]; if (std::sscanf(d.substr(pos, e - pos).c_str(), "%7s %d %7s %d", a, &rows, b, &cols) != 4 || std::string(a) != "-Y" || std::string(b) != "+X") { err = "unsupported Radiance orientation"; return false; }
    pos = e + 1;
    std::vector<uint8_t> px((size_t)rows * cols * 4);
    const uint8_t *buf = (const uint8_t *)d.data(); const size_t n = d.size();
    for (int y = 0; y < rows; ++y) {
        uint8_t *row = &px[(size_t)y * cols * 4];
        if (pos + 4 > n) { err = "truncated Radiance data"; return false; }
        if (cols < 8 || cols > 0x7FFF || buf[pos] != 2 || buf[pos + 1] != 2 || (buf[pos + 2] & 0x80)) { if (pos + (size_t)4 * cols > n) { err = "truncated Radiance data"; return false; } std::memcpy(row, buf + pos, (size_t)4 * cols); pos += (size_t)4 * cols; continue; }
        if ((((int)buf[pos + 2]) << 8 | (int)buf[pos + 3]) != cols) { err = "scanline width mismatch"; return false; }
        pos += 4;
        for (int c = 0; c < 4; ++c) for (int x = 0; x < cols;) {
            if (pos >= n) { err = "truncated Radiance data"; return false; }
            int k = buf[pos++];
            if (k > 128) { k -= 128; if (pos >= n || x + k > cols) { err = "bad Radiance run"; return false; } for (int i = 0; i < k; ++i) row[4 * (x + i) + c] = buf[pos]; ++pos; }
            else { if (pos + (size_t)k > n || x + k > cols || k == 0) { err = "bad Radiance run"; return false; } for (int i = 0; i < k; ++i) row[4 * (x + i) + c] = buf[pos + i]; pos += (size_t)k; }
            x += k;
        }
    }
    rgb.resize((size_t)rows * cols * 3);
    for (size_t p = 0; p < (size_t)rows * cols; ++p) { const int ex = px[4 * p + 3]; const float sc = ex == 0 ? 0.0f : std::ldexp(1.0f, ex - 136); for (int c = 0; c < 3; ++c) rgb[3 * p + c] = (float)px[4 * p + c] * sc; }
    return true;
}
void distribution_1d(const float *f, int n, float *cdf, float &func_int) { // Distribution1D::new (sampling.rs:134-157)
    cdf[0] = 0.0f;
    float acc = 0.0f;
    for (int i = 0; i < n; ++i) { acc = acc + f[i] / (float)n; cdf[i + 1] = acc; }
    func_int = cdf[n];
    if (func_int == 0.0f) for (int i = 1; i <= n; ++i) cdf[i] = (float)i / (float)n;
    else for (int i = 1; i <= n; ++i) cdf[i] = cdf[i] / func_int;
}
bool invert4(const float m[16], float out[16]) { // binary64 Gauss-Jordan
    double a[4][8];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { a[i][j] = m[4 * i + j]; a[i][4 + j] = i == j ? 1.0 : 0.0; }
    for (int c = 0; c < 4; ++c) {
        int p = c; for (int r = c + 1; r < 4; ++r) if (std::fabs(a[r][c]) > std::fabs(a[p][c])) p = r;
        if (a[p][c] == 0.0) return false;
        if (p != c) for (int j = 0; j < 8; ++j) std::swap(a[p][j], a[c][j]);
        const double d = a[c][c]; for (int j = 0; j < 8; ++j) a[c][j] /= d;
        for (int r = 0; r < 4; ++r) if (r != c) { const double f = a[r][c]; if (f != 0.0) for (int j = 0; j < 8; ++j) a[r][j] -= f * a[c][j]; }
    }
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) out[4 * i + j] = (float)a[i][4 + j];
    return true;
}
bool add_infinite_light(RenderScene &s, std::vector<float> texels, int rows, int cols, const float l2w[16], std::string &err) { // light.rs:348-398
    const int32_t lmap = add_image_texture(s, std::move(texels), rows, cols, 3, PTRS_WRAP_REPEAT);
    const TexImage &ti = *s.images.back();
    const int width = 2 * ti.cols[0], height = 2 * ti.rows[0];
    const float f_width = 0.5f / (float)std::min(width, height);
    const float level = (float)ti.levels.size() - 1.0f + (float)std::log2(std::max((double)f_width, 1e-8));
    if (!(level < 0.0f)) { err = "environment maps whose distribution lookup is not at level 0 are not supported"; return false; }
    auto d = std::make_unique<EnvDistribution>();
    d->nu = width; d->nv = height;
    d->func.resize((size_t)width * height); d->cdf.resize((size_t)(width + 1) * height); d->func_int.resize((size_t)height); d->marg_cdf.resize((size_t)height + 1);
    const int R = ti.rows[0], Cn = ti.cols[0]; const std::vector<float> &l0 = ti.levels[0];
    for (int v = 0; v < height; ++v) {
        const float vp = ((float)v + 0.5f) / (float)height;
        const float sin_theta = (float)std::sin((double)(3.14159274101257324f * vp));
        const float t = vp * (float)R - 0.5f; const float t0f = std::floor(t); const float dt = t - t0f; const long t0 = (long)t0f;
        for (int u = 0; u < width; ++u) {
            const float up = ((float)u + 0.5f) / (float)width;
            const float sx = up * (float)Cn - 0.5f; const float s0f = std::floor(sx); const float ds = sx - s0f; const long s0 = (long)s0f;
            float rgb[3];
            for (int c = 0; c < 3; ++c) { // MIPMap::triangle(0, st) with Repeat wrap (texture.rs:413-428)
                auto tx = [&](long si, long tj) { return l0[((size_t)wrap_index(tj, R, PTRS_WRAP_REPEAT) * Cn + (size_t)wrap_index(si, Cn, PTRS_WRAP_REPEAT)) * 3 + c]; };
                const float A = tx(s0, t0) * (1.0f - ds) * (1.0f - dt), B = tx(s0, t0 + 1) * (1.0f - ds) * dt, C2 = tx(s0 + 1, t0) * ds * (1.0f - dt), D = tx(s0 + 1, t0 + 1) * ds * dt;
                rgb[c] = ((A + B) + C2) + D;
            }
            const float lum = (rgb[0] * 0.212671f + rgb[1] * 0.715160f) + rgb[2] * 0.072169f;
            d->func[(size_t)v * width + u] = sin_theta * lum;
        }
        distribution_1d(&d->func[(size_t)v * width], width, &d->cdf[(size_t)v * (width + 1)], d->func_int[(size_t)v]);
    }
    distribution_1d(d->func_int.data(), height, d->marg_cdf.data(), d->marg_func_int);
    PtrsLight L{}; L.kind = PTRS_LIGHT_INFINITE; L.ke_tex = -1; L.lmap_tex = lmap;
    std::memcpy(L.light_to_world, l2w, 64);
    if (!invert4(l2w, L.world_to_light)) { err = "singular light_to_world"; return false; }
    L.dist_nu = width; L.dist_nv = height; L.dist_func = d->func.data(); L.dist_cdf = d->cdf.data(); L.dist_func_int = d->func_int.data(); L.marg_cdf = d->marg_cdf.data(); L.marg_func_int = d->marg_func_int;
    s.env_dists.push_back(std::move(d));
    s.lights.push_back(L);
    return true;
}

} // namespace

// ---- pieces the Mitsuba importer (ptrs_host.cpp) shares with this file ----------------------------------------------
bool load_rgb8_image(const std::string &path, int &rows, int &cols, std::vector<uint8_t> &rgb, std::string &err) {
    std::string data; Image8 img;
    if (!read_file(path, data)) { err = "cannot open " + path; return false; }
    if (!decode_image(data, img, err)) return false;
    if (!img.supported || img.ch != 3) { err = "unsupported image format for texture"; return false; } // anything but DynamicImage::ImageRgb8 (mitsuba.rs:61-63)
    rows = img.h; cols = img.w; rgb = std::move(img.px);
    return true;
}
int32_t add_spectrum_image_texture(RenderScene &s, const std::vector<uint8_t> &rgb8, int rows, int cols, int wrap, const float uvmap[4]) {
    std::vector<float> v((size_t)rows * cols * 3); // ImageTexture::<Spectrum>::new, scale 1, gamma = true (texture.rs:123-147)
    for (size_t k = 0; k < v.size(); ++k) v[k] = 1.0f * inverse_gamma_correct((float)rgb8[k] / 255.0f);
    const int32_t t = add_image_texture(s, std::move(v), rows, cols, 3, wrap);
    PtrsTexture &x = s.textures[(size_t)t]; x.su = uvmap[0]; x.sv = uvmap[1]; x.du = uvmap[2]; x.dv = uvmap[3];
    return t;
}
bool add_env_light_from_file(RenderScene &s, const std::string &hdr_path, const float light_to_world[16], std::string &err) {
    std::vector<float> rgb; int rows, cols;
    if (!read_rgbe(hdr_path, rgb, rows, cols, err)) return false;
    return add_infinite_light(s, std::move(rgb), rows, cols, light_to_world, err);
}
void matmul4(const float a[16], const float b[16], float out[16]) {
    M4 x, y; std::memcpy(x.m, a, 64); std::memcpy(y.m, b, 64);
    const M4 r = mul(x, y); std::memcpy(out, r.m, 64);
}

bool import_gltf(const std::string &path, int rw, int rh, bool default_lights, const std::string &env_map_path, Camera &camera, RenderScene &scene, std::string &err) {
    Importer imp;
    scene = RenderScene();
    imp.scene = &scene;
    auto bail = [&]() { err = imp.err.empty() ? "glTF import failed" : imp.err; return false; };
    if (!imp.load(path)) return bail();
    imp.materials.push_back(add_mat(scene, PTRS_MAT_MATTE, {const_tex(scene, 3, 1.0f, 1.0f, 1.0f)})); // default_material (gltf.rs:22-28)
    if (const JVal *ms = imp.doc.get("materials")) for (size_t k = 0; k < ms->size(); ++k) { int32_t m; if (!imp.material(ms->at(k), m)) return bail(); imp.materials.push_back(m); }
    const M4 I = ident();
    const JVal *scenes = imp.doc.get("scenes");
    if (scenes) for (size_t k = 0; k < scenes->size(); ++k) if (const JVal *ns = scenes->at(k).get("nodes")) for (size_t j = 0; j < ns->size(); ++j) if (!imp.populate(I, (int)ns->at(j).n)) return bail();
    if (scene.meshes.empty()) { err = "glTF file without triangle meshes"; return false; }
    for (auto &l : imp.deferred) scene.lights.push_back(l);
    if (default_lights) {
        if (env_map_path.empty()) { err = "--default_lights needs --env_map FILE.hdr: the reference's bundled HDR is not shipped"; return false; }
        std::vector<float> rgb; int rows, cols;
        if (!read_rgbe(env_map_path, rgb, rows, cols, err)) return false;
        // UnitQuaternion::from_euler_angles(-pi/2, 0, 0): the env map is z-up, the scene y-up (gltf.rs:553-562)
        const float c = (float)std::cos(-3.14159265358979323846 / 2), sn = (float)std::sin(-3.14159265358979323846 / 2);
        const float l2w[16] = {1, 0, 0, 0, 0, c, -sn, 0, 0, sn, c, 0, 0, 0, 0, 1};
        if (!add_infinite_light(scene, std::move(rgb), rows, cols, l2w, err)) return false;
    }
    bool found = false;
    if (scenes) for (size_t k = 0; k < scenes->size() && !found; ++k) if (const JVal *ns = scenes->at(k).get("nodes")) for (size_t j = 0; j < ns->size() && !found; ++j) found = imp.find_camera(I, (int)ns->at(j).n, rw, rh, camera);
    if (!found) { // get_default_camera (common/importer/gltf.rs:68-85): binary64 look-at like gltf.py:default_camera
        double hi[3] = {-1e300, -1e300, -1e300};
        for (auto &m : scene.meshes) for (size_t i = 0; i < m.pos.size(); ++i) hi[i % 3] = std::max(hi[i % 3], (double)m.pos[i]);
        const double en = std::sqrt(hi[0] * hi[0] + hi[1] * hi[1] + hi[2] * hi[2]);
        const double f[3] = {-hi[0] / en, -hi[1] / en, -hi[2] / en}, up[3] = {0, 1, 0};
        double sv[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
        const double sn2 = std::sqrt(sv[0] * sv[0] + sv[1] * sv[1] + sv[2] * sv[2]); for (double &x : sv) x /= sn2;
        const double u[3] = {sv[1] * f[2] - sv[2] * f[1], sv[2] * f[0] - sv[0] * f[2], sv[0] * f[1] - sv[1] * f[0]};
        float r[3][3]; for (int k = 0; k < 3; ++k) { r[k][0] = (float)sv[k]; r[k][1] = (float)u[k]; r[k][2] = (float)-f[k]; }
        float q[4]; quat_from_rotation(r, q);
        const float tr[3] = {(float)hi[0], (float)hi[1], (float)hi[2]};
        make_camera_perspective(q, tr, (float)rw / (float)rh, (float)(3.14159265358979323846 / 2) * ((float)rh / (float)rw), 0.01f, 10000.0f, rw, rh, camera);
    }
    return true;
}

} // namespace ptrs_host
