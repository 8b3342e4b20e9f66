// Host check of csrc/scene_request.h (tests/test_scene_request_host.py builds and runs it under the sanitizers): the rules of a scene
// description with their codes, texts and order, the decisions of scene creation -- accelerator, kernel variant, the curved /
// cylinders flags, the SAH constant, where a tree goes -- against literals, find_occluders against literal rooms and against a
// float64 segment test over drawn scenes, and the host tables built whole for a brute-force and a BVH scene.
// Prints one JSON line: {"checks": N, "failures": M, "scenes": S, "scenes_with_drops": D, "dropped": P, "segments": G}.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "scene_request.h"

static int checks = 0, failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        ++checks;                                                     \
        if (!(cond)) {                                                \
            ++failures;                                               \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);   \
        }                                                             \
    } while (0)

static const uint32_t LDS = 163840, STACKS = 4 * 1024 * 4;  // the LDS of a workgroup, the traversal stacks of a 1024-thread workgroup
static const float NaN = NAN, Inf = INFINITY;

// ---- scenes -----------------------------------------------------------------------------------------------------------------------
struct V {
    double x, y, z;
};
static V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V operator*(double s, V a) { return {s * a.x, s * a.y, s * a.z}; }
static double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static V unit(V a) { return (1.0 / std::sqrt(dot(a, a))) * a; }

static pbrt_prim planar(uint32_t type, V v0, V e1, V e2, uint32_t material = 0, int32_t emitter = -1) {
    pbrt_prim p;
    std::memset(&p, 0, sizeof p);
    const float g[9] = {(float)v0.x, (float)v0.y, (float)v0.z, (float)e1.x, (float)e1.y, (float)e1.z, (float)e2.x, (float)e2.y, (float)e2.z};
    std::memcpy(p.g, g, sizeof g);
    const V n = unit(cross(V{g[3], g[4], g[5]}, V{g[6], g[7], g[8]}));  // the float32 of the unit normal of the float32 edges
    p.g[9] = (float)n.x, p.g[10] = (float)n.y, p.g[11] = (float)n.z;
    p.type = type, p.material = material, p.emitter = emitter;
    return p;
}
static pbrt_prim quad(V v0, V e1, V e2, uint32_t material = 0, int32_t emitter = -1) { return planar(PBRT_PRIM_PARALLELOGRAM, v0, e1, e2, material, emitter); }
static pbrt_prim tri(V v0, V e1, V e2, uint32_t material = 0, int32_t emitter = -1) { return planar(PBRT_PRIM_TRIANGLE, v0, e1, e2, material, emitter); }
static pbrt_prim sphere(V c, double r, uint32_t material = 0) {
    pbrt_prim p;
    std::memset(&p, 0, sizeof p);
    p.g[0] = (float)c.x, p.g[1] = (float)c.y, p.g[2] = (float)c.z, p.g[3] = (float)r;
    p.type = PBRT_PRIM_SPHERE, p.material = material, p.emitter = -1;
    return p;
}
// a cone / cylinder from its world -> object rows (m | t)
static pbrt_prim quadric(uint32_t type, const double m[3][3], const double t[3], uint32_t material = 0) {
    pbrt_prim p;
    std::memset(&p, 0, sizeof p);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) p.g[4 * r + c] = (float)m[r][c];
        p.g[4 * r + 3] = (float)t[r];
    }
    p.type = type, p.material = material, p.emitter = -1;
    return p;
}
static pbrt_prim scaled_quadric(uint32_t type, double s, V at, uint32_t material = 0) {  // object = (world - at) / s
    const double m[3][3] = {{1 / s, 0, 0}, {0, 1 / s, 0}, {0, 0, 1 / s}}, t[3] = {-at.x / s, -at.y / s, -at.z / s};
    return quadric(type, m, t, material);
}
static pbrt_material material(uint32_t type, float p0 = 0.5f, float eta = 0.2f, float k = 3.0f) {
    pbrt_material m;
    m.type = type;
    m.p[0] = p0;
    for (int i = 1; i < 4; ++i) m.p[i] = eta, m.p[i + 3] = k;
    return m;
}
static pbrt_emitter point_light(V at) {
    pbrt_emitter e;
    std::memset(&e, 0, sizeof e);
    e.type = PBRT_EMIT_POINT;
    e.radiance[0] = e.radiance[1] = e.radiance[2] = 1.0f;
    e.pos[0] = (float)at.x, e.pos[1] = (float)at.y, e.pos[2] = (float)at.z;
    return e;
}
static pbrt_emitter area_light(uint32_t first, uint32_t count) {
    pbrt_emitter e;
    std::memset(&e, 0, sizeof e);
    e.type = PBRT_EMIT_AREA;
    e.first = first, e.count = count, e.area = 1.0f;
    return e;
}

struct Scene {
    std::vector<pbrt_prim> prims;
    std::vector<pbrt_material> mats;
    std::vector<pbrt_emitter> emitters;
    std::vector<uint32_t> light_prims;
    std::vector<float> light_cdf, vn;
    uint32_t accel = PBRT_ACCEL_AUTO;
    pbrt_scene_desc desc() const {
        pbrt_scene_desc d;
        std::memset(&d, 0, sizeof d);
        d.n_prims = (uint32_t)prims.size(), d.prims = prims.data();
        d.n_materials = (uint32_t)mats.size(), d.materials = mats.data();
        d.n_emitters = (uint32_t)emitters.size(), d.emitters = emitters.empty() ? nullptr : emitters.data();
        d.n_light_prims = (uint32_t)light_prims.size();
        d.light_prims = light_prims.empty() ? nullptr : light_prims.data();
        d.light_cdf = light_cdf.empty() ? nullptr : light_cdf.data();
        d.accel = accel;
        d.vertex_normals = vn.empty() ? nullptr : vn.data();
        return d;
    }
};

// what the maker says of a description: "" (taken), or code and text
struct Said {
    int code;
    std::string text;
};
static Said said(const pbrt_scene_desc *d, bool out = true, SceneRequest *keep = nullptr) {
    SceneRequest local, *rq = keep ? keep : &local;
    const int rc = scene_request(rq, d, out, LDS, STACKS);
    CHECK(rc == rq->why.code && (rc == PBRT_OK) == (rq->why.text[0] == 0));
    return {rc, rq->why.text};
}
static Said said(const Scene &sc, SceneRequest *keep = nullptr) {
    const pbrt_scene_desc d = sc.desc();
    return said(&d, true, keep);
}
static bool is(const Said &s, int code, const std::string &text) {
    if (s.code == code && s.text == text) return true;
    std::fprintf(stderr, "  got %d \"%s\", want %d \"%s\"\n", s.code, s.text.c_str(), code, text.c_str());
    return false;
}
static std::string at(const char *what, size_t i, const char *rest) { return std::string(what) + " " + std::to_string(i) + ": " + rest; }

// ---- the rule table -----------------------------------------------------------------------------------------------------------------
static const char *T_NULL = "invalid argument: d && out";
static const char *T_COUNTS = "invalid argument: d->n_prims > 0 && d->prims && d->n_materials > 0 && d->materials";
static const char *T_EMITTERS = "invalid argument: d->n_emitters == 0 || d->emitters";
static const char *T_LIGHTS = "invalid argument: d->n_light_prims == 0 || (d->light_prims && d->light_cdf)";
static const char *T_ACCEL = "invalid argument: d->accel <= PBRT_ACCEL_BVH_GLOBAL";
static const char *T_CONE = "cone needs an invertible, finite world -> object matrix";
static const char *T_CYL = "cylinder needs an invertible, finite world -> object matrix";
static const char *T_MAT = "material out of range", *T_EMIT = "emitter out of range";
static const char *T_ALPHA = "roughconductor alpha must be finite and > 0";
static const char *T_ETA = "conductor eta must be finite and >= 0", *T_K = "conductor k must be finite and >= 0";
static const char *T_RANGE = "light primitive range out of bounds", *T_AREA = "area lights need triangle/parallelogram primitives";
static const char *T_ETYPE = "unknown type";
static const int INV = PBRT_E_INVALID, UNS = PBRT_E_UNSUPPORTED;

// five primitives of every class, three materials, three emitters (an area light of the two planar primitives, two point lights)
static Scene base_scene() {
    Scene sc;
    sc.prims = {sphere({0, 0, 0}, 0.5, 2), quad({-1, 1, -1}, {2, 0, 0}, {0, 0, 2}, 0, 0), scaled_quadric(PBRT_PRIM_CONE, 0.5, {1, 0, 0}, 1),
                tri({-1, 1.5, -1}, {2, 0, 0}, {0, 0, 2}, 1, 0), scaled_quadric(PBRT_PRIM_CYLINDER, 0.5, {-1, 0, 0}, 2)};
    sc.mats = {material(PBRT_MAT_DIFFUSE), material(PBRT_MAT_ROUGHCONDUCTOR, 0.1f), material(PBRT_MAT_CONDUCTOR_FRESNEL)};
    sc.emitters = {area_light(0, 2), point_light({0, 0.5, 0}), point_light({0.5, 0.5, 0})};
    sc.light_prims = {1, 3};
    sc.light_cdf = {0.6f, 1.0f};
    sc.vn.assign(5 * 9, 0.0f);
    return sc;
}

static void rule_table() {
    const Scene ok = base_scene();
    CHECK(is(said(ok), PBRT_OK, ""));
    pbrt_scene_desc d = ok.desc();
    CHECK(is(said(nullptr), INV, T_NULL) && is(said(&d, false), INV, T_NULL) && is(said(nullptr, false), INV, T_NULL));
    // counts and pointers
    auto broken = [&](auto edit) {
        pbrt_scene_desc e = ok.desc();
        edit(e);
        return said(&e);
    };
    CHECK(is(broken([](pbrt_scene_desc &e) { e.n_prims = 0; }), INV, T_COUNTS));
    CHECK(is(broken([](pbrt_scene_desc &e) { e.prims = nullptr; }), INV, T_COUNTS));
    CHECK(is(broken([](pbrt_scene_desc &e) { e.n_materials = 0; }), INV, T_COUNTS));
    CHECK(is(broken([](pbrt_scene_desc &e) { e.materials = nullptr; }), INV, T_COUNTS));
    CHECK(is(broken([](pbrt_scene_desc &e) { e.emitters = nullptr; }), INV, T_EMITTERS));
    CHECK(is(broken([](pbrt_scene_desc &e) { e.light_prims = nullptr; }), INV, T_LIGHTS));
    CHECK(is(broken([](pbrt_scene_desc &e) { e.light_cdf = nullptr; }), INV, T_LIGHTS));
    CHECK(is(broken([](pbrt_scene_desc &e) { e.accel = 4; }), INV, T_ACCEL));
    CHECK(is(broken([](pbrt_scene_desc &e) { e.accel = 0xffffffffu; }), INV, T_ACCEL));
    for (uint32_t a = 0; a < 4; ++a) CHECK(is(broken([a](pbrt_scene_desc &e) { e.accel = a; }), PBRT_OK, ""));
    // no emitters, no light primitives: null tables are fine
    Scene dark = ok;
    dark.emitters.clear(), dark.light_prims.clear(), dark.light_cdf.clear();
    for (pbrt_prim &p : dark.prims) p.emitter = -1;
    CHECK(is(said(dark), PBRT_OK, ""));
    // per primitive, at the first, a middle and the last record
    for (size_t i : {size_t(0), size_t(2), size_t(4)}) {
        Scene sc = ok;
        sc.prims[i].type = 5;
        CHECK(is(said(sc), UNS, at("primitive", i, "type 5 is not supported")));
        sc.prims[i].type = 0x80000000u;
        CHECK(is(said(sc), UNS, at("primitive", i, "type 2147483648 is not supported")));
        for (uint32_t type : {PBRT_PRIM_CONE, PBRT_PRIM_CYLINDER}) {
            const char *text = type == PBRT_PRIM_CONE ? T_CONE : T_CYL;
            sc = ok;
            sc.prims[i] = scaled_quadric(type, 0.5, {0, 0, 0});
            CHECK(is(said(sc), PBRT_OK, ""));
            sc.prims[i].g[8] = sc.prims[i].g[9] = sc.prims[i].g[10] = 0.0f;  // a zero row: singular
            CHECK(is(said(sc), INV, at("primitive", i, text)));
            sc.prims[i] = scaled_quadric(type, 0.5, {0, 0, 0});
            sc.prims[i].g[5] = NaN;
            CHECK(is(said(sc), INV, at("primitive", i, text)));
            sc.prims[i] = scaled_quadric(type, 0.5, {0, 0, 0});
            sc.prims[i].g[3] = Inf;  // an infinite translation: the frame is not finite
            CHECK(is(said(sc), INV, at("primitive", i, text)));
        }
        sc = ok;
        sc.prims[i].material = 3;
        CHECK(is(said(sc), INV, at("primitive", i, T_MAT)));
        sc.prims[i].material = 2;
        CHECK(is(said(sc), PBRT_OK, ""));
        sc.prims[i].emitter = 3;
        CHECK(is(said(sc), INV, at("primitive", i, T_EMIT)));
        sc.prims[i].emitter = -7;  // any negative index: none
        CHECK(is(said(sc), PBRT_OK, ""));
    }
    // materials
    for (size_t i : {size_t(0), size_t(1), size_t(2)}) {
        Scene sc = ok;
        for (float alpha : {0.0f, -0.1f, NaN, Inf}) {
            sc.mats[i] = material(PBRT_MAT_ROUGHCONDUCTOR, alpha);
            CHECK(is(said(sc), INV, at("material", i, T_ALPHA)));
            sc.mats[i] = material(PBRT_MAT_CONDUCTOR_FRESNEL, alpha);  // (its p[0] is not read)
            CHECK(is(said(sc), PBRT_OK, ""));
            sc.mats[i] = material(PBRT_MAT_DIFFUSE, alpha, NaN, -1.0f);  // (nor any field of the other types)
            CHECK(is(said(sc), PBRT_OK, ""));
        }
        for (uint32_t type : {PBRT_MAT_ROUGHCONDUCTOR, PBRT_MAT_CONDUCTOR_FRESNEL})
            for (int k = 1; k < 7; ++k)
                for (float bad : {-1e-6f, NaN, Inf, -Inf}) {
                    sc.mats[i] = material(type);
                    sc.mats[i].p[k] = bad;
                    CHECK(is(said(sc), INV, at("material", i, k < 4 ? T_ETA : T_K)));
                    sc.mats[i].p[k] = 0.0f;
                    CHECK(is(said(sc), PBRT_OK, ""));
                }
    }
    // emitters
    for (size_t i : {size_t(0), size_t(1), size_t(2)}) {
        Scene sc = ok;
        sc.emitters[i] = area_light(0, 0);
        CHECK(is(said(sc), INV, at("emitter", i, T_RANGE)));
        sc.emitters[i] = area_light(1, 2);
        CHECK(is(said(sc), INV, at("emitter", i, T_RANGE)));
        sc.emitters[i] = area_light(2, 1);
        CHECK(is(said(sc), INV, at("emitter", i, T_RANGE)));
        sc.emitters[i] = area_light(1, 1);
        CHECK(is(said(sc), PBRT_OK, ""));
        if (i) sc.emitters[0] = area_light(0, 1);  // (so that only emitter i reads light_prims[1])
        for (uint32_t curved : {0u, 2u, 4u, 5u}) {  // a sphere, a cone, a cylinder, an index past the table
            sc.light_prims[1] = curved;
            CHECK(is(said(sc), UNS, at("emitter", i, T_AREA)));
        }
        sc = ok;
        sc.emitters[i].type = 2;
        CHECK(is(said(sc), INV, at("emitter", i, T_ETYPE)));
    }
    // vertex normals
    for (size_t i : {size_t(0), size_t(22), size_t(44)})
        for (float bad : {NaN, Inf, -Inf}) {
            Scene sc = ok;
            sc.vn[i] = bad;
            CHECK(is(said(sc), INV, "vertex_normals: entry " + std::to_string(i) + " is not finite"));
        }
    // two rules broken: the earlier one speaks
    Scene sc = ok;
    sc.accel = 4, sc.vn[7] = NaN;
    CHECK(is(said(sc), INV, "vertex_normals: entry 7 is not finite"));
    sc.emitters[2].type = 9;
    CHECK(is(said(sc), INV, at("emitter", 2, T_ETYPE)));
    sc.emitters[0] = area_light(0, 3);
    CHECK(is(said(sc), INV, at("emitter", 0, T_RANGE)));
    sc.mats[2].p[6] = -1.0f;
    CHECK(is(said(sc), INV, at("material", 2, T_K)));
    sc.mats[1].p[0] = 0.0f;
    CHECK(is(said(sc), INV, at("material", 1, T_ALPHA)));
    sc.prims[4].emitter = 3;
    CHECK(is(said(sc), INV, at("primitive", 4, T_EMIT)));
    sc.prims[4].material = 9;
    CHECK(is(said(sc), INV, at("primitive", 4, T_MAT)));
    sc.prims[4].g[0] = NaN;
    CHECK(is(said(sc), INV, at("primitive", 4, T_CYL)));
    sc.prims[2].material = 3;
    CHECK(is(said(sc), INV, at("primitive", 2, T_MAT)));
    sc.prims[2].g[0] = sc.prims[2].g[1] = sc.prims[2].g[2] = 0.0f;
    CHECK(is(said(sc), INV, at("primitive", 2, T_CONE)));
    sc.prims[2].type = 6;
    CHECK(is(said(sc), UNS, at("primitive", 2, "type 6 is not supported")));
    sc.prims[1].emitter = 5;
    CHECK(is(said(sc), INV, at("primitive", 1, T_EMIT)));
    d = sc.desc();
    d.light_cdf = nullptr;
    CHECK(is(said(&d), INV, T_LIGHTS));
    d.emitters = nullptr;
    CHECK(is(said(&d), INV, T_EMITTERS));
    d.n_materials = 0;
    CHECK(is(said(&d), INV, T_COUNTS));
    CHECK(is(said(&d, false), INV, T_NULL));
    // the material rule on its own, as pbrt_scene_update_material and the BSDF leaf operators call it
    Refusal why;
    CHECK(material_rule(material(PBRT_MAT_ROUGHCONDUCTOR, 0.3f), 0, &why) == PBRT_OK && why.code == PBRT_OK && why.text[0] == 0);
    CHECK(material_rule(material(PBRT_MAT_ROUGHCONDUCTOR, 0.0f), 17, &why) == INV && why.code == INV && at("material", 17, T_ALPHA) == why.text);
    CHECK(material_rule(material(PBRT_MAT_CONDUCTOR_FRESNEL, 0.0f, -1.0f), 0, &why) == INV && at("material", 0, T_ETA) == why.text);
    CHECK(material_is_glossy(PBRT_MAT_ROUGHCONDUCTOR) && material_is_glossy(PBRT_MAT_CONDUCTOR_FRESNEL));
    for (uint32_t t : {PBRT_MAT_DIFFUSE, PBRT_MAT_CONDUCTOR, PBRT_MAT_DIELECTRIC, PBRT_MAT_ULTRA, PBRT_MAT_NONE, 7u}) CHECK(!material_is_glossy(t));
}

// ---- the decisions ------------------------------------------------------------------------------------------------------------------
// n unit quads in a row, one diffuse material, a point light
static Scene row_of_quads(uint32_t n, uint32_t accel = PBRT_ACCEL_AUTO) {
    Scene sc;
    for (uint32_t i = 0; i < n; ++i) sc.prims.push_back(quad({(double)i, 0, 0}, {0.5, 0, 0}, {0, 0.5, 0}));
    sc.mats = {material(PBRT_MAT_DIFFUSE)};
    sc.emitters = {point_light({0, 0, 3})};
    sc.accel = accel;
    return sc;
}
static SceneRequest request_of(const Scene &sc, uint32_t lds_limit = LDS) {
    SceneRequest rq;
    const pbrt_scene_desc d = sc.desc();
    CHECK(scene_request(&rq, &d, true, lds_limit, STACKS) == PBRT_OK);
    rq.d = nullptr;  // (the description was a local)
    return rq;
}

static void decisions() {
    // the accelerator
    CHECK(!request_of(row_of_quads(32)).want_bvh && request_of(row_of_quads(33)).want_bvh && !request_of(row_of_quads(1)).want_bvh);
    CHECK(!request_of(row_of_quads(33, PBRT_ACCEL_BRUTE)).want_bvh && !request_of(row_of_quads(500, PBRT_ACCEL_BRUTE)).want_bvh);
    CHECK(request_of(row_of_quads(1, PBRT_ACCEL_BVH)).want_bvh && request_of(row_of_quads(1, PBRT_ACCEL_BVH_GLOBAL)).want_bvh);
    // small_tables and the brute-force variant
    CHECK(brute_variant(true, false) == ACCEL_K_BRUTE && brute_variant(true, true) == ACCEL_K_BRUTE_BIG);
    CHECK(brute_variant(false, false) == ACCEL_K_BRUTE_BIG && brute_variant(false, true) == ACCEL_K_BRUTE_BIG);
    auto brute = [](const Scene &sc, bool small, bool glossy = false) {
        const SceneRequest rq = request_of(sc);
        const SceneFacts &f = rq.facts;
        return !rq.want_bvh && f.small_tables == small && f.glossy == glossy && f.accel_kernel == brute_variant(small, glossy) && f.curved &&
               !f.cylinders && f.lds_bytes == 0 && f.bvh_depth == 0 && f.mat_types.size() == sc.mats.size();
    };
    CHECK(brute(row_of_quads(32), true) && brute(row_of_quads(32, PBRT_ACCEL_BRUTE), true) && brute(row_of_quads(33, PBRT_ACCEL_BRUTE), false));
    Scene sc = row_of_quads(8);
    sc.mats.assign(32, material(PBRT_MAT_DIFFUSE));
    CHECK(brute(sc, true));
    sc.mats.assign(33, material(PBRT_MAT_DIFFUSE));
    CHECK(brute(sc, false));
    sc = row_of_quads(8);
    sc.emitters.assign(32, point_light({0, 0, 3}));
    CHECK(brute(sc, true));
    sc.emitters.assign(33, point_light({0, 0, 3}));
    CHECK(brute(sc, false));
    sc = row_of_quads(8);
    sc.prims[3] = scaled_quadric(PBRT_PRIM_CONE, 0.5, {0, 2, 0});
    CHECK(brute(sc, false));
    sc.prims[3] = scaled_quadric(PBRT_PRIM_CYLINDER, 0.5, {0, 2, 0});
    CHECK(brute(sc, false));
    sc.prims[3] = sphere({0, 2, 0}, 0.5);
    CHECK(brute(sc, true));
    sc.vn.assign(8 * 9, 0.0f);
    CHECK(brute(sc, false));
    for (uint32_t type : {PBRT_MAT_ROUGHCONDUCTOR, PBRT_MAT_CONDUCTOR_FRESNEL}) {
        sc = row_of_quads(8);
        sc.mats = {material(PBRT_MAT_DIFFUSE), material(type)};
        CHECK(brute(sc, true, true));
        sc.prims[3] = scaled_quadric(PBRT_PRIM_CONE, 0.5, {0, 2, 0});
        CHECK(brute(sc, false, true));
    }
    // a material update: glossy and the variant follow the types, small_tables stays
    SceneRequest rq = request_of(row_of_quads(8));
    SceneFacts f = rq.facts;
    f.mat_types[0] = PBRT_MAT_ROUGHCONDUCTOR;
    scene_set_glossy(&f);
    CHECK(f.glossy && f.accel_kernel == ACCEL_K_BRUTE_BIG && f.small_tables);
    f.mat_types[0] = PBRT_MAT_CONDUCTOR;
    scene_set_glossy(&f);
    CHECK(!f.glossy && f.accel_kernel == ACCEL_K_BRUTE);
    // BVH scenes: curved / cylinders by primitive class; glossy leaves their kernel alone
    auto bvh_flags = [](pbrt_prim p, bool curved, bool cylinders) {
        Scene s = row_of_quads(3, PBRT_ACCEL_BVH);
        s.prims[1] = p;
        s.mats = {material(PBRT_MAT_ROUGHCONDUCTOR)};
        const SceneRequest q = request_of(s);
        return q.want_bvh && q.facts.curved == curved && q.facts.cylinders == cylinders && !q.facts.small_tables && q.facts.glossy &&
               q.facts.accel_kernel == ACCEL_K_BVH_GLOBAL;
    };
    CHECK(bvh_flags(quad({0, 1, 0}, {1, 0, 0}, {0, 1, 0}), false, false) && bvh_flags(tri({0, 1, 0}, {1, 0, 0}, {0, 1, 0}), false, false));
    CHECK(bvh_flags(sphere({0, 2, 0}, 0.5), true, false) && bvh_flags(scaled_quadric(PBRT_PRIM_CONE, 0.5, {0, 2, 0}), true, false));
    CHECK(bvh_flags(scaled_quadric(PBRT_PRIM_CYLINDER, 0.5, {0, 2, 0}), true, true));
    // the SAH constant: 100 leaf records are 4000 bytes
    CHECK(request_of(row_of_quads(100), 0).sure_global && !request_of(row_of_quads(100), 4000).sure_global);
    CHECK(request_of(row_of_quads(100), 3999).sure_global && request_of(row_of_quads(101), 4000).sure_global);
    CHECK(!request_of(row_of_quads(100, PBRT_ACCEL_BVH)).sure_global && request_of(row_of_quads(100, PBRT_ACCEL_BVH_GLOBAL)).sure_global);
    // the placement: 11 nodes and 100 primitives are 11 * 56 + 100 * 40 = 4616 bytes, 4624 rounded up to 16; beside 16384 bytes of
    // stacks and 1024 of slack they need 22024
    uint32_t lds_bytes = 7;
    CHECK(tree_placement(11, 100, 3, 22023, STACKS, PBRT_ACCEL_BVH, &lds_bytes) == ACCEL_K_BVH_GLOBAL && lds_bytes == 7);
    CHECK(tree_placement(11, 100, 3, 22024, STACKS, PBRT_ACCEL_BVH, &lds_bytes) == ACCEL_K_BVH_LDS && lds_bytes == 4624);
    lds_bytes = 7;
    CHECK(tree_placement(11, 100, 3, 22025, STACKS, PBRT_ACCEL_AUTO, &lds_bytes) == ACCEL_K_BVH_LDS && lds_bytes == 4624);
    CHECK(tree_placement(10, 100, 3, LDS, STACKS, PBRT_ACCEL_BVH, &lds_bytes) == ACCEL_K_BVH_LDS && lds_bytes == 4560);  // (a multiple of 16 stays)
    CHECK(tree_placement(11, 100, 3, 22024, STACKS + 1, PBRT_ACCEL_BVH, &lds_bytes) == ACCEL_K_BVH_GLOBAL);
    CHECK(tree_placement(11, 100, 3, LDS, STACKS, PBRT_ACCEL_BVH_GLOBAL, &lds_bytes) == ACCEL_K_BVH_GLOBAL);
    CHECK(tree_placement(11, 100, 3, 0, STACKS, PBRT_ACCEL_BVH, &lds_bytes) == ACCEL_K_BVH_GLOBAL);
    // the traversal state: 32 levels, 2^24 - 2 nodes, 2^27 - 1 primitives
    CHECK(tree_placement(11, 100, 32, LDS, STACKS, PBRT_ACCEL_BVH, &lds_bytes) == ACCEL_K_BVH_LDS);
    CHECK(tree_placement(11, 100, 33, LDS, STACKS, PBRT_ACCEL_BVH, &lds_bytes) == -1);
    CHECK(tree_placement((1u << 24) - 2, 100, 3, LDS, STACKS, PBRT_ACCEL_BVH, &lds_bytes) == ACCEL_K_BVH_GLOBAL);
    CHECK(tree_placement((1u << 24) - 1, 100, 3, LDS, STACKS, PBRT_ACCEL_BVH, &lds_bytes) == -1);
    CHECK(tree_placement(11, (1u << 27) - 1, 3, LDS, STACKS, PBRT_ACCEL_BVH, &lds_bytes) == ACCEL_K_BVH_GLOBAL);
    CHECK(tree_placement(11, 1u << 27, 3, LDS, STACKS, PBRT_ACCEL_BVH_GLOBAL, &lds_bytes) == -1);
    // ... and as the stage reports it
    sc = row_of_quads(3, PBRT_ACCEL_BVH);
    const pbrt_scene_desc d = sc.desc();
    CHECK(scene_request(&rq, &d, true, LDS, STACKS) == PBRT_OK);
    SceneTables t;
    t.b4.nodes.resize(2);
    t.b4.depth = 33;
    CHECK(scene_place(&rq, t) == UNS && rq.why.code == UNS && std::string(rq.why.text) == "BVH depth 33 / 2 nodes exceed the traversal state");
}

// ---- find_occluders -----------------------------------------------------------------------------------------------------------------
static std::vector<pbrt_prim> room(double h = 1.0) {  // floor, ceiling, back, left, right of [-1, 1]^3, open towards +z
    return {quad({-1, -h, -1}, {2, 0, 0}, {0, 0, 2}), quad({-1, h, -1}, {0, 0, 2}, {2, 0, 0}), quad({-1, -h, -1}, {0, 2 * h, 0}, {2, 0, 0}),
            quad({-1, -h, -1}, {0, 0, 2}, {0, 2 * h, 0}), quad({1, -h, -1}, {0, 2 * h, 0}, {0, 0, 2})};
}
static std::vector<pbrt_prim> box(V lo, V hi) {
    const V d = hi - lo, x{d.x, 0, 0}, y{0, d.y, 0}, z{0, 0, d.z};
    return {quad(lo, x, y), quad(lo, y, z), quad(lo, z, x), quad(hi, -1.0 * y, -1.0 * x), quad(hi, -1.0 * z, -1.0 * y), quad(hi, -1.0 * x, -1.0 * z)};
}
static bool same(const pbrt_prim &a, const pbrt_prim &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void occluder_literals() {
    Scene sc;
    sc.prims = room();
    sc.mats = {material(PBRT_MAT_DIFFUSE)};
    sc.emitters = {point_light({0.2, 0.5, 0.1})};
    pbrt_scene_desc d = sc.desc();
    CHECK(find_occluders(&d).empty());
    sc.emitters[0] = point_light({0.2, 1.5, 0.1});  // the light above the ceiling: the ceiling is between it and the room
    d = sc.desc();
    std::vector<pbrt_prim> occ = find_occluders(&d);
    CHECK(occ.size() == 1 && same(occ[0], sc.prims[1]));
    sc.emitters[0] = point_light({0.2, 0.5, 0.1});
    const std::vector<pbrt_prim> b = box({-0.5, -0.9, -0.5}, {0.1, -0.2, 0.3});  // (floating: a face ON the floor's plane would go too)
    sc.prims.insert(sc.prims.begin() + 2, b.begin(), b.end());  // (between the walls: the list keeps its order)
    d = sc.desc();
    occ = find_occluders(&d);
    CHECK(occ.size() == 6);
    for (size_t k = 0; k < 6 && k < occ.size(); ++k) CHECK(same(occ[k], b[k]));
    // a light quad below the ceiling as the only emitter: geometry on both sides of it, and it never occludes
    sc.prims = room();
    sc.prims.push_back(quad({-0.3, 0.9, -0.3}, {0, 0, 0.6}, {0.6, 0, 0}, 0, 0));
    sc.emitters = {area_light(0, 1)};
    sc.light_prims = {5};
    sc.light_cdf = {1.0f};
    d = sc.desc();
    CHECK(find_occluders(&d).empty());
    sc.emitters.push_back(point_light({0, 0, 0}));  // with a second emitter it does
    d = sc.desc();
    occ = find_occluders(&d);
    CHECK(occ.size() == 1 && same(occ[0], sc.prims[5]));
    sc.emitters = {area_light(0, 2)};  // ... and as one of two primitives of the light
    sc.light_prims = {5, 0};
    sc.light_cdf = {0.5f, 1.0f};
    d = sc.desc();
    occ = find_occluders(&d);
    CHECK(occ.size() == 1 && same(occ[0], sc.prims[5]));
    // spheres, cones and cylinders are always kept; one that pokes through a wall's plane keeps the wall
    sc = Scene();
    sc.prims = room();
    sc.prims.push_back(sphere({0, 0, 0}, 0.4));
    sc.prims.push_back(scaled_quadric(PBRT_PRIM_CONE, 0.3, {0.5, -0.5, 0}));      // a disc of radius 0.3 in z = 0, apex at z = 0.3: inside
    sc.prims.push_back(scaled_quadric(PBRT_PRIM_CYLINDER, 0.3, {-0.5, 0.8, 0}));  // its discs reach y = 1.1: through the ceiling's plane
    sc.mats = {material(PBRT_MAT_DIFFUSE)};
    sc.emitters = {point_light({0, 0.5, 0})};
    d = sc.desc();
    occ = find_occluders(&d);
    CHECK(occ.size() == 4 && same(occ[0], sc.prims[1]) && same(occ[1], sc.prims[5]) && same(occ[2], sc.prims[6]) && same(occ[3], sc.prims[7]));
    sc.prims[7] = scaled_quadric(PBRT_PRIM_CYLINDER, 0.3, {-0.5, 0.6, 0});  // ... y = 0.9: inside
    d = sc.desc();
    CHECK(find_occluders(&d).size() == 3);
}

// The property: no segment between two points of the OTHER primitives or of the point emitters crosses the interior of a dropped
// primitive.  Both sides in float64 on the float32 records: the points from v0 + u e1 + v e2, centre + r w, and the object -> world
// map of a cone / cylinder inverted here; the dropped primitive's plane through v0 with the normal e1 x e2.
// The rounding margin, EPS: find_occluders measures sides against the STORED normal, the float32 of that unit normal -- each
// component off by at most 2^-24, so for a point within 16 of v0 (the scenes are drawn inside [-4, 4]^3: at most 8 sqrt(3) < 14)
// the two sides differ by at most 16 sqrt(3) 2^-24 < 1.7e-6; the float64 evaluation itself (a dozen operations on numbers below 16,
// inverses of matrices with condition below 20) adds less than 1e-12.  A segment counts as crossing when its end points are more
// than EPS on either side and it meets the plane inside the primitive, more than 1e-9 (in u, v) from its edges.
static const double EPS = 2e-6;

struct Frame {  // object -> world of a cone / cylinder record: world = o + x a + y b + z c
    V o, a, b, c;
};
static Frame object_to_world(const pbrt_prim &P) {
    const V r0{P.g[0], P.g[1], P.g[2]}, r1{P.g[4], P.g[5], P.g[6]}, r2{P.g[8], P.g[9], P.g[10]};
    const double det = dot(r0, cross(r1, r2));
    Frame f;
    f.a = (1.0 / det) * cross(r1, r2);  // the columns of the inverse: the dual basis of the rows
    f.b = (1.0 / det) * cross(r2, r0);
    f.c = (1.0 / det) * cross(r0, r1);
    f.o = -1.0 * ((double)P.g[3] * f.a + (double)P.g[7] * f.b + (double)P.g[11] * f.c);
    return f;
}
// points of a primitive: its corners or extremes along `n` first, then drawn ones
static void points_of(const pbrt_prim &Q, V n, std::mt19937 &rng, int drawn, std::vector<V> *out) {
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const double two_pi = 6.283185307179586;
    if (Q.type == PBRT_PRIM_TRIANGLE || Q.type == PBRT_PRIM_PARALLELOGRAM) {
        const V v0{Q.g[0], Q.g[1], Q.g[2]}, e1{Q.g[3], Q.g[4], Q.g[5]}, e2{Q.g[6], Q.g[7], Q.g[8]};
        out->insert(out->end(), {v0, v0 + e1, v0 + e2});
        if (Q.type == PBRT_PRIM_PARALLELOGRAM) out->push_back(v0 + e1 + e2);
        for (int k = 0; k < drawn; ++k) {
            double u = U(rng), v = U(rng);
            if (Q.type == PBRT_PRIM_TRIANGLE && u + v > 1.0) u = 1.0 - u, v = 1.0 - v;
            out->push_back(v0 + u * e1 + v * e2);
        }
    } else if (Q.type == PBRT_PRIM_SPHERE) {
        const V c{Q.g[0], Q.g[1], Q.g[2]};
        const double r = Q.g[3];
        out->insert(out->end(), {c + r * unit(n), c - r * unit(n)});
        std::normal_distribution<double> N(0.0, 1.0);
        for (int k = 0; k < drawn; ++k) out->push_back(c + r * unit(V{N(rng), N(rng), N(rng)}));
    } else {  // cone: the disc z = 0 shrinking to the apex z = 1; cylinder: the unit disc along z = 0 .. 1
        const Frame f = object_to_world(Q);
        const bool cone = Q.type == PBRT_PRIM_CONE;
        const double phi0 = std::atan2(dot(f.b, n), dot(f.a, n));  // where the rim reaches furthest along n
        for (double phi : {phi0, phi0 + 0.5 * two_pi}) {
            const V rim = std::cos(phi) * f.a + std::sin(phi) * f.b;
            out->push_back(f.o + rim);
            out->push_back(cone ? f.o + f.c : f.o + rim + f.c);
        }
        for (int k = 0; k < drawn; ++k) {
            const double phi = two_pi * U(rng), z = U(rng), rho = (k & 1) ? 1.0 : std::sqrt(U(rng));  // on the side, or on a cap / inside
            const double s = rho * (cone ? 1.0 - z : 1.0);
            out->push_back(f.o + (s * std::cos(phi)) * f.a + (s * std::sin(phi)) * f.b + z * f.c);
        }
    }
}
static bool crosses(const pbrt_prim &P, V A, V B) {
    const V v0{P.g[0], P.g[1], P.g[2]}, e1{P.g[3], P.g[4], P.g[5]}, e2{P.g[6], P.g[7], P.g[8]}, n = unit(cross(e1, e2));
    const double sa = dot(n, A - v0), sb = dot(n, B - v0);
    if (!((sa > EPS && sb < -EPS) || (sa < -EPS && sb > EPS))) return false;
    const V X = A + (sa / (sa - sb)) * (B - A), w = X - v0;
    const double a11 = dot(e1, e1), a12 = dot(e1, e2), a22 = dot(e2, e2), b1 = dot(w, e1), b2 = dot(w, e2), det = a11 * a22 - a12 * a12;
    const double u = (b1 * a22 - b2 * a12) / det, v = (a11 * b2 - a12 * b1) / det, m = 1e-9;
    return u > m && v > m && (P.type == PBRT_PRIM_TRIANGLE ? u + v < 1.0 - m : (u < 1.0 - m && v < 1.0 - m));
}

static int n_scenes = 0, n_scenes_with_drops = 0, n_dropped = 0;
static long long n_segments = 0;

static void occluder_property() {
    std::mt19937 rng(20240611);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    auto in = [&](double lo, double hi) { return lo + (hi - lo) * U(rng); };
    auto vec = [&](double r) { return V{in(-r, r), in(-r, r), in(-r, r)}; };
    for (int s = 0; s < 2400; ++s) {
        Scene sc;
        sc.mats = {material(PBRT_MAT_DIFFUSE)};
        // the interior, within [-3.8, 3.8]^3: planar primitives in any pose, spheres, a cone and a cylinder in affine poses
        const int n_planar = 2 + (int)(rng() % 5);
        for (int k = 0; k < n_planar; ++k) {
            const V v0 = vec(2.0), e1 = vec(0.9), e2 = vec(0.9);
            if (std::sqrt(dot(cross(e1, e2), cross(e1, e2))) < 0.05) continue;  // (a sliver: its normal is badly conditioned)
            sc.prims.push_back(rng() % 2 ? quad(v0, e1, e2) : tri(v0, e1, e2));
        }
        for (int k = (int)(rng() % 3); k > 0; --k) sc.prims.push_back(sphere(vec(2.0), in(0.2, 0.7)));
        for (uint32_t type : {PBRT_PRIM_CONE, PBRT_PRIM_CYLINDER}) {
            if (rng() % 2) continue;
            // object -> world: a rotation about a drawn axis times a non-uniform, sometimes mirrored scale; the record is its inverse
            const V ax = unit(vec(1.0) + V{0.01, 0.02, 0.03}), u0 = unit(cross(ax, V{0.3, -0.5, 0.8})), w0 = cross(ax, u0), at = vec(1.5);
            const double ang = in(0, 6.28), sx = in(0.3, 1.1) * (rng() % 2 ? -1 : 1), sy = in(0.3, 1.1), sz = in(0.4, 1.3);
            const V a = sx * (std::cos(ang) * u0 + std::sin(ang) * w0), b = sy * (std::cos(ang) * w0 - std::sin(ang) * u0), c = sz * ax;
            const double det = dot(a, cross(b, c));
            const V r0 = (1.0 / det) * cross(b, c), r1 = (1.0 / det) * cross(c, a), r2 = (1.0 / det) * cross(a, b);
            const double m[3][3] = {{r0.x, r0.y, r0.z}, {r1.x, r1.y, r1.z}, {r2.x, r2.y, r2.z}}, t[3] = {-dot(r0, at), -dot(r1, at), -dot(r2, at)};
            sc.prims.push_back(quadric(type, m, t));
        }
        for (int k = 1 + (int)(rng() % 2); k > 0 && s % 8; --k) sc.emitters.push_back(point_light(vec(2.5)));
        // walls: quads over [-3, 3]^2 -- every other one within 0.15 of where the interior ends on that side, so that its outermost
        // primitive or emitter, whatever it is, decides whether the wall can go; the others 1.6 .. 3.9 from the origin: around all of
        // that or through it, and from 3 on on one side of each other -- and some tilted inwards
        const std::vector<pbrt_prim> interior = sc.prims;
        for (int k = (int)(rng() % 4); k > 0; --k) {
            const int axis = (int)(rng() % 3);
            const double sign = rng() % 2 ? -1 : 1, tilt = rng() % 3 ? 0.0 : in(-0.6, 0.6);
            const V along{axis == 0 ? sign : 0.0, axis == 1 ? sign : 0.0, axis == 2 ? sign : 0.0};
            std::vector<V> ends;
            for (const pbrt_prim &Q : interior) points_of(Q, along, rng, 0, &ends);
            for (const pbrt_emitter &e : sc.emitters) ends.push_back(V{e.pos[0], e.pos[1], e.pos[2]});
            double reach = 0.0;
            for (V p : ends) reach = std::max(reach, dot(along, p));
            const double w = sign * (k % 2 && tilt == 0.0 ? std::min(reach + in(-0.15, 0.15), 3.9) : in(1.6, 3.9));
            double v0[3] = {-3.0, -3.0, -3.0}, e1[3] = {0, 0, 0}, e2[3] = {0, 0, 0};
            v0[axis] = w;
            e1[(axis + 1) % 3] = 6.0, e1[axis] = (w > 0 ? -1 : 1) * std::fabs(tilt) * 6.0;
            e2[(axis + 2) % 3] = 6.0;
            sc.prims.insert(sc.prims.begin() + (long)(rng() % (sc.prims.size() + 1)), quad({v0[0], v0[1], v0[2]}, {e1[0], e1[1], e1[2]}, {e2[0], e2[1], e2[2]}));
        }
        if (sc.prims.empty()) continue;
        const pbrt_scene_desc d = sc.desc();
        SceneRequest rq;
        CHECK(scene_request(&rq, &d, true, LDS, STACKS) == PBRT_OK);
        const std::vector<pbrt_prim> occ = find_occluders(&d);
        // the list is a sub-sequence of the primitives, and only planar ones are dropped
        std::vector<size_t> dropped;
        size_t o = 0;
        for (size_t i = 0; i < sc.prims.size(); ++i) {
            if (o < occ.size() && same(occ[o], sc.prims[i])) {
                ++o;
                continue;
            }
            dropped.push_back(i);
            CHECK(sc.prims[i].type == PBRT_PRIM_TRIANGLE || sc.prims[i].type == PBRT_PRIM_PARALLELOGRAM);
        }
        CHECK(o == occ.size());
        ++n_scenes;
        n_scenes_with_drops += !dropped.empty();
        n_dropped += (int)dropped.size();
        for (size_t i : dropped) {
            const pbrt_prim &P = sc.prims[i];
            const V n = cross(V{P.g[3], P.g[4], P.g[5]}, V{P.g[6], P.g[7], P.g[8]});
            std::vector<V> pts;
            for (size_t j = 0; j < sc.prims.size(); ++j)
                if (j != i) points_of(sc.prims[j], n, rng, 12, &pts);
            for (const pbrt_emitter &e : sc.emitters) pts.push_back(V{e.pos[0], e.pos[1], e.pos[2]});
            long long crossing = 0;
            for (size_t a = 0; a < pts.size(); ++a)
                for (size_t b = a + 1; b < pts.size(); ++b) crossing += crosses(P, pts[a], pts[b]);
            n_segments += (long long)(pts.size() * (pts.size() - 1) / 2);
            CHECK(crossing == 0);
        }
    }
    CHECK(n_scenes >= 2000 && 3 * n_scenes_with_drops >= n_scenes);
    // the test itself can see a crossing: a wall between two points
    const pbrt_prim wall = quad({-1, -1, 0}, {2, 0, 0}, {0, 2, 0});
    CHECK(crosses(wall, {0.2, 0.3, -1}, {0.1, -0.4, 2}) && !crosses(wall, {0.2, 0.3, 1}, {0.1, -0.4, 2}) && !crosses(wall, {3, 0.3, -1}, {3, -0.4, 2}));
}

// ---- the host tables ------------------------------------------------------------------------------------------------------------------
static void host_tables() {
    // brute force: a room with a box, a sphere, a cone and a triangle between them (not class-ordered)
    Scene sc;
    sc.prims = room();
    const std::vector<pbrt_prim> b = box({-0.5, -0.9, -0.5}, {0.1, -0.2, 0.3});
    sc.prims.insert(sc.prims.end(), b.begin(), b.end());
    sc.prims.push_back(sphere({0.5, 0, 0}, 0.3));
    sc.prims.push_back(tri({-0.2, 0.2, -0.2}, {0.4, 0, 0}, {0, 0.3, 0.1}));
    sc.prims.push_back(scaled_quadric(PBRT_PRIM_CONE, 0.3, {0.5, -0.5, 0.5}));
    sc.mats = {material(PBRT_MAT_DIFFUSE)};
    sc.emitters = {point_light({0, 0.5, 0})};
    pbrt_scene_desc d = sc.desc();
    SceneRequest rq;
    CHECK(scene_request(&rq, &d, true, LDS, STACKS) == PBRT_OK && !rq.want_bvh);
    SceneTables t;
    scene_tables(rq, &t);
    const std::vector<pbrt_prim> occ = find_occluders(&d);
    CHECK(t.occ.size() == 9 && t.occ.size() == occ.size() && std::memcmp(t.occ.data(), occ.data(), occ.size() * sizeof(pbrt_prim)) == 0);
    CHECK(t.runs == cut_prim_runs(sc.prims.data(), sc.prims.size()) && t.occ_runs == cut_prim_runs(occ.data(), occ.size()));
    CHECK(t.runs == (std::vector<uint32_t>{11u << 2 | PRIM_RUN_QUAD, 1u << 2 | PRIM_RUN_CURVED, 1u << 2 | PRIM_RUN_TRI, 1u << 2 | PRIM_RUN_CURVED}));
    CHECK(t.prim_ord == 0 && t.occ_ord == 0 && t.b4.nodes.empty() && t.leaves.empty());
    CHECK(scene_place(&rq, t) == PBRT_OK && rq.facts.accel_kernel == ACCEL_K_BRUTE_BIG && rq.facts.lds_bytes == 0);
    // the same scene class-ordered: quads, the triangle, the curved ones
    std::swap(sc.prims[11], sc.prims[12]);
    d = sc.desc();
    CHECK(scene_request(&rq, &d, true, LDS, STACKS) == PBRT_OK);
    t = SceneTables();
    scene_tables(rq, &t);
    const uint32_t cnt[3] = {11, 1, 2}, occ_cnt[3] = {6, 1, 2};
    CHECK(t.prim_ord == prim_ord_pack(cnt) && t.occ_ord == prim_ord_pack(occ_cnt) && t.prim_ord != 0 && t.occ_ord != 0);
    CHECK(t.runs.size() == 3 && t.occ_runs.size() == 3);
    // a BVH scene: 300 drawn triangles and a sphere, a cone and a cylinder among them
    std::mt19937 rng(7);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    sc = Scene();
    for (int k = 0; k < 300; ++k) {
        const V c{2.5 * U(rng), 2.5 * U(rng), 2.5 * U(rng)};
        sc.prims.push_back(tri(c, {0.3 * U(rng), 0.3 * U(rng), 0.3 * U(rng)}, {0.3 * U(rng), 0.3 * U(rng), 0.3 * U(rng)}));
    }
    sc.prims[17] = sphere({0.5, 0, 0}, 0.3);
    sc.prims[99] = scaled_quadric(PBRT_PRIM_CONE, 0.3, {0.5, -1, 0.5});
    sc.prims[200] = scaled_quadric(PBRT_PRIM_CYLINDER, 0.3, {-0.5, 1, 0.5});
    sc.mats = {material(PBRT_MAT_DIFFUSE)};
    for (uint32_t lds_limit : {LDS, 11999u, 0u}) {  // a tree for the LDS; leaf records alone too large; no LDS known
        d = sc.desc();
        CHECK(scene_request(&rq, &d, true, lds_limit, STACKS) == PBRT_OK && rq.want_bvh && rq.sure_global == (lds_limit != LDS));
        t = SceneTables();
        scene_tables(rq, &t);
        CHECK(t.occ.empty() && t.runs.empty() && t.occ_runs.empty() && t.prim_ord == 0 && t.occ_ord == 0);
        CHECK(!t.b4.nodes.empty() && t.b4.depth >= 2 && t.b4.depth <= BVH_STK_MAX && t.leaves.size() == 300);
        std::vector<int> seen(300, 0);
        for (const HostLeafPrim &L : t.leaves) {
            const uint32_t id = L.meta & 0x0fffffffu;
            CHECK(id < 300 && (L.meta >> 28) == sc.prims[id].type && std::memcmp(L.g, sc.prims[id].g, sizeof L.g) == 0);
            if (id < 300) ++seen[id];
        }
        CHECK(std::count(seen.begin(), seen.end(), 1) == 300);
        uint32_t n_leaf_refs = 0;  // every leaf record is referenced by exactly one leaf of the tree
        for (const HostNode4 &N : t.b4.nodes)
            for (uint32_t c : N.child)
                if (c & 0x80000000u) n_leaf_refs += (c >> 27) & 15u;
        CHECK(n_leaf_refs == 300);
        CHECK(scene_place(&rq, t) == PBRT_OK && rq.facts.bvh_depth == t.b4.depth && rq.facts.curved && rq.facts.cylinders);
        const size_t image = t.b4.nodes.size() * 56 + 300 * 40;
        CHECK(image + STACKS + 1024 <= LDS);
        if (lds_limit == LDS)
            CHECK(rq.facts.accel_kernel == ACCEL_K_BVH_LDS && rq.facts.lds_bytes == ((image + 15) / 16) * 16);
        else
            CHECK(rq.facts.accel_kernel == ACCEL_K_BVH_GLOBAL && rq.facts.lds_bytes == 0);
    }
}

int main() {
    rule_table();
    decisions();
    occluder_literals();
    occluder_property();
    host_tables();
    std::printf("{\"checks\": %d, \"failures\": %d, \"scenes\": %d, \"scenes_with_drops\": %d, \"dropped\": %d, \"segments\": %lld}\n", checks,
                failures, n_scenes, n_scenes_with_drops, n_dropped, n_segments);
    return failures ? 1 : 0;
}
