// Host program around csrc/tile_cull.h (tests/test_tile_cull_host.py builds it with the address and undefined-behaviour sanitizers
// and runs it on its own): the keep words of named cases -- a camera, a film cut into blocks of 64 region indices as the first
// bounce's waves see it (film_key.h region_index), a primitive list.  Prints one JSON object:
//   {"cases": {name: {"cam": [17 numbers], "prims": [[type, 12 numbers], ...], "blocks": [[x0, y0, x1, y1, word], ...]}},
//    "bits": all (block, primitive) bits, "cleared": how many of them are clear, "cleared_share": their share}
// The test casts the oracle's camera rays against the oracle's primitive tests and holds every cleared bit to them.
//
// With one argument the cases come from that file instead (tests/tile_cull_util.py write_cases: the camera, the primitives and the
// block rectangles of a render on the device, whose keep words tests/test_gpu_tile_keep_words.py compares with the ones printed
// here), as whitespace-separated tokens, floats as %.9g so that the float32 values are exact:
//   case NAME  cam <12 matrix entries> tan_half_fov_x near far film_w film_h  prims N <N x (type, 12 numbers)>
//   rects M <M x (x0 y0 x1 y1)>  -- absolute film pixels, inclusive
// and the output has the same shape, one word per rectangle.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "tile_cull.h"

struct Rect {
    uint32_t x0, y0, x1, y1;
};
struct Case {
    std::string name;
    pbrt_camera cam;
    std::vector<pbrt_prim> prims;
    std::vector<Rect> rects;  // empty: the blocks of the whole film (block_rects)
};

static pbrt_prim planar(uint32_t type, float x, float y, float z, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z) {
    pbrt_prim P = {};
    const float g[9] = {x, y, z, e1x, e1y, e1z, e2x, e2y, e2z};
    for (int k = 0; k < 9; ++k) P.g[k] = g[k];
    P.type = type;
    P.emitter = -1;
    return P;
}
static pbrt_prim quad(float x, float y, float z, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z) {
    return planar(PBRT_PRIM_PARALLELOGRAM, x, y, z, e1x, e1y, e1z, e2x, e2y, e2z);
}
static pbrt_prim tri(float x, float y, float z, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z) {
    return planar(PBRT_PRIM_TRIANGLE, x, y, z, e1x, e1y, e1z, e2x, e2y, e2z);
}
static pbrt_prim sphere(float x, float y, float z, float r) {
    pbrt_prim P = {};
    P.g[0] = x;
    P.g[1] = y;
    P.g[2] = z;
    P.g[3] = r;
    P.type = PBRT_PRIM_SPHERE;
    P.emitter = -1;
    return P;
}

// the Cornell box of tests/scenes/cbox.xml as Scene.flatten() hands it to the library (the test compares): luminaire, floor,
// ceiling, back wall, the walls at x = -1 and x = +1, the mirror ball and the glass ball
static std::vector<pbrt_prim> cbox() {
    return {quad(0.25f, 0.99000001f, -0.25f, 0, 0, 0.5f, -0.5f, 0, 0), quad(-1, -1, 1, 2, 0, 0, 0, 0, -2),
            quad(1, 1, -1, 0, 0, 2, -2, 0, 0),                         quad(1, -1, -1, 0, 2, 0, -2, 0, 0),
            quad(-1, 1, -1, 0, 0, 2, 0, -2, 0),                        quad(1, -1, 1, 0, 2, 0, 0, 0, -2),
            sphere(-0.300000012f, -0.5f, 0.200000003f, 0.5f),          sphere(0.5f, -0.75f, -0.200000003f, 0.25f)};
}

// Mitsuba's look_at: columns (left, up, dir, origin) of the camera-to-world matrix
static pbrt_camera look_at(double ox, double oy, double oz, double tx, double ty, double tz, double ux, double uy, double uz, uint32_t w,
                           uint32_t h, float near_clip = 0.001f, float far_clip = 100.0f) {
    auto norm = [](double *v) {
        const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        for (int k = 0; k < 3; ++k) v[k] /= l;
    };
    double dir[3] = {tx - ox, ty - oy, tz - oz}, up[3] = {ux, uy, uz};
    norm(dir);
    double left[3] = {up[1] * dir[2] - up[2] * dir[1], up[2] * dir[0] - up[0] * dir[2], up[0] * dir[1] - up[1] * dir[0]};
    norm(left);
    const double nup[3] = {dir[1] * left[2] - dir[2] * left[1], dir[2] * left[0] - dir[0] * left[2], dir[0] * left[1] - dir[1] * left[0]};
    const double org[3] = {ox, oy, oz};
    pbrt_camera c = {};
    for (int r = 0; r < 3; ++r) {
        c.to_world[4 * r + 0] = (float)left[r];
        c.to_world[4 * r + 1] = (float)nup[r];
        c.to_world[4 * r + 2] = (float)dir[r];
        c.to_world[4 * r + 3] = (float)org[r];
    }
    c.tan_half_fov_x = 0.357143372f;  // cbox.xml: fov 39.3077 on the smaller axis
    c.near_clip = near_clip;
    c.far_clip = far_clip;
    c.film_w = w;
    c.film_h = h;
    return c;
}

// the pixel of region index pr: the inverse of region_index restated (film_key.h region_pixel is the library's), region = the whole film
static void pixel_of(uint32_t pr, uint32_t rw, uint32_t tile_rows, uint32_t *x, uint32_t *y) {
    const bool tiled = pr < tile_rows * rw;
    const uint32_t num = tiled ? pr >> 3 : pr, q = num / rw;
    *x = num - q * rw;
    *y = tiled ? (q << 3) + (pr & 7u) : q;
}

// the blocks of 64 region indices of a region that is the whole film: the bounding box of the 64 pixels of each
static std::vector<Rect> block_rects(uint32_t rw, uint32_t rh) {
    const uint32_t tile_rows = rh & ~7u, n_blocks = rw * rh / 64;
    std::vector<Rect> out;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        Rect r = {~0u, ~0u, 0, 0};
        for (uint32_t k = 0; k < 64; ++k) {
            uint32_t x, y;
            pixel_of(b * 64 + k, rw, tile_rows, &x, &y);
            r.x0 = x < r.x0 ? x : r.x0;
            r.x1 = x > r.x1 ? x : r.x1;
            r.y0 = y < r.y0 ? y : r.y0;
            r.y1 = y > r.y1 ? y : r.y1;
        }
        out.push_back(r);
    }
    return out;
}

static std::vector<Case> builtin_cases() {
    std::vector<Case> cases;
    cases.push_back({"cbox_64", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 64, 64), cbox()});
    cases.push_back({"cbox_48x80", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 48, 80), cbox()});
    cases.push_back({"cbox_12x16", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 12, 16), cbox()});  // blocks straddle the 8-row bands
    cases.push_back({"rotated", look_at(2.5, 1.5, 3.0, 0.1, -0.2, 0, 0.2, 1, 0.1, 64, 64), cbox()});
    cases.push_back({"near_plane", look_at(0.999, 0.1, 0.5, -1, -0.3, -0.4, 0, 1, 0, 32, 32), cbox()});  // 1e-3 from the wall x = 1
    cases.push_back({"in_plane", look_at(0, -1, 3, 0, 0, 0, 0, 1, 0, 32, 32), cbox()});                   // in the floor's plane y = -1
    cases.push_back({"far_1e4", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 32, 32, 0.001f, 1e4f), cbox()});
    cases.push_back({"far_1e6", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 32, 32, 0.001f, 1e6f), cbox()});
    cases.push_back({"sliver", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 32, 32),
                     {tri(-0.9f, -0.4f, 0, 1.8f, 0.7f, 0, 1.8f, 0.7002f, 0), tri(-0.5f, 0.3f, -0.5f, 1e-3f, 0, 0, 0, 0.6f, 0.3f),
                      tri(-0.6f, -0.6f, 0.2f, 1.1f, 0.1f, 0, 0.2f, 0.9f, 0.3f)}});
    // a sphere that touches the ray through the film's centre, the corner of four tiles, from the side; and one that touches the
    // film's corner ray
    cases.push_back({"tangent_sphere", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 32, 32),
                     {sphere(0.3f, 0, 0, 0.3f), sphere(0, -0.25f, 1, 0.25f),
                      sphere(-0.357143372f * 4.0f - 0.2f * 1.1187f, 0.357143372f * 4.0f + 0.2f * 1.1187f, 0, 0.2f)}});
    cases.push_back({"sphere_around_camera", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 32, 32),
                     {sphere(0, 0, 4, 0.5f), sphere(0.2f, 0, 4.1f, 0.3f), sphere(0, 0, 0, 10), sphere(0.4f, 0.1f, 3.6f, 0.39f)}});
    cases.push_back({"behind_camera", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 32, 32),
                     {quad(-1, -1, 6, 2, 0, 0, 0, 2, 0), sphere(0, 0, 7, 1), sphere(0, 0, 4.6f, 0.5f), tri(-1, -1, 4.01f, 2, 0, 0, 0, 2, 0),
                      quad(-3, -1, 5, 6, 0, -2, 0, 2, 0), sphere(0.3f, 0.2f, 0, 0.4f)}});
    // regions with a row-major tail below the last full 8-row band, or with no band at all (tile_rows == 0)
    cases.push_back({"cbox_16x12", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 16, 12), cbox()});  // two 8 x 8 blocks and one 16 x 4 tail block
    cases.push_back({"cbox_32x10", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 32, 10), cbox()});  // four 8 x 8 blocks and one 32 x 2 tail block
    cases.push_back({"cbox_64x9", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 64, 9), cbox()});    // the tail is a single row
    cases.push_back({"cbox_48x4", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 48, 4), cbox()});    // no band; the middle block spans two rows
    cases.push_back({"cbox_128x1", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 128, 1), cbox()});  // no band; two blocks
    cases.push_back({"cbox_20x16", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 20, 16), cbox()});  // width no multiple of 8; no tail
    cases.push_back({"cbox_4x16", look_at(0, 0, 4, 0, 0, 0, 0, 1, 0, 4, 16), cbox()});    // one block: the whole region
    return cases;
}

// the cases of a file (the format is at the top); false: the file does not parse
static bool read_cases(const char *path, std::vector<Case> *cases) {
    std::ifstream in(path);
    std::string tok;
    auto word = [&](const char *want) { return (in >> tok) && tok == want; };
    auto real = [&](float *v) {
        if (!(in >> tok)) return false;
        char *end = nullptr;
        *v = std::strtof(tok.c_str(), &end);
        return end != tok.c_str() && *end == 0;
    };
    auto count = [&](uint32_t *v) {
        if (!(in >> tok)) return false;
        char *end = nullptr;
        const unsigned long long u = std::strtoull(tok.c_str(), &end, 10);
        *v = (uint32_t)u;
        return end != tok.c_str() && *end == 0 && u <= 0xffffffffull;
    };
    while (in >> tok) {
        Case c = {};
        if (tok != "case" || !(in >> c.name) || !word("cam")) return false;
        for (int k = 0; k < 12; ++k)
            if (!real(&c.cam.to_world[k])) return false;
        if (!real(&c.cam.tan_half_fov_x) || !real(&c.cam.near_clip) || !real(&c.cam.far_clip) || !count(&c.cam.film_w) || !count(&c.cam.film_h))
            return false;
        uint32_t n = 0;
        if (!word("prims") || !count(&n) || n > 32) return false;
        for (uint32_t i = 0; i < n; ++i) {
            pbrt_prim P = {};
            P.emitter = -1;
            if (!count(&P.type)) return false;
            for (int k = 0; k < 12; ++k)
                if (!real(&P.g[k])) return false;
            c.prims.push_back(P);
        }
        if (!word("rects") || !count(&n) || n == 0 || n > (1u << 20)) return false;
        for (uint32_t i = 0; i < n; ++i) {
            Rect r;
            if (!count(&r.x0) || !count(&r.y0) || !count(&r.x1) || !count(&r.y1)) return false;
            c.rects.push_back(r);
        }
        cases->push_back(c);
    }
    return !cases->empty();
}

int main(int argc, char **argv) {
    std::vector<Case> cases;
    if (argc > 2 || (argc == 2 && !read_cases(argv[1], &cases))) {
        std::fprintf(stderr, "usage: %s [case file]; %s\n", argv[0], argc == 2 ? "the file does not parse" : "one argument at the most");
        return 2;
    }
    if (argc < 2) cases = builtin_cases();

    unsigned long long bits = 0, cleared = 0;
    std::printf("{\"cases\": {");
    for (size_t ci = 0; ci < cases.size(); ++ci) {
        const Case &c = cases[ci];
        const uint32_t rw = c.cam.film_w, rh = c.cam.film_h;
        const std::vector<Rect> rects = c.rects.empty() ? block_rects(rw, rh) : c.rects;
        std::printf("%s\"%s\": {\"cam\": [", ci ? ", " : "", c.name.c_str());
        for (int k = 0; k < 12; ++k) std::printf("%.9g, ", c.cam.to_world[k]);
        std::printf("%.9g, %.9g, %.9g, %u, %u], \"prims\": [", c.cam.tan_half_fov_x, c.cam.near_clip, c.cam.far_clip, rw, rh);
        for (size_t i = 0; i < c.prims.size(); ++i) {
            std::printf("%s[%u", i ? ", " : "", c.prims[i].type);
            for (int k = 0; k < 12; ++k) std::printf(", %.9g", c.prims[i].g[k]);
            std::printf("]");
        }
        std::printf("], \"blocks\": [");
        for (size_t b = 0; b < rects.size(); ++b) {
            const Rect &r = rects[b];
            uint32_t word = 0;
            for (size_t i = 0; i < c.prims.size(); ++i) {
                const bool keep = tile_cull_keep(c.cam, r.x0, r.y0, r.x1, r.y1, c.prims[i]);
                word |= (keep ? 1u : 0u) << i;
                ++bits;
                cleared += keep ? 0 : 1;
            }
            std::printf("%s[%u, %u, %u, %u, %u]", b ? ", " : "", r.x0, r.y0, r.x1, r.y1, word);
        }
        std::printf("]}");
    }
    std::printf("}, \"bits\": %llu, \"cleared\": %llu, \"cleared_share\": %.4f}\n", bits, cleared, bits ? (double)cleared / (double)bits : 0.0);
    return 0;
}
