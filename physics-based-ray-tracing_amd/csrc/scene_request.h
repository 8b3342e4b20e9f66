// One scene-creation request: "make this pbrt_scene_desc resident", as pbrt_scene_create hands it to its stages (pbrt_api.hip) -- the
// rules the description must keep, each written once and all of them ahead of any device call, the facts the kernels are chosen by,
// each derived once, and everything that is uploaded, built in host vectors.  The material rule is the one of
// pbrt_scene_update_material and the BSDF leaf operators as well.  Plain host code (no HIP), so that
// tests/native/scene_request_check.cpp can build it on its own.  The constants of the kernels the decisions depend on live here
// (device_scene.h includes this header); what depends on a kernel's workgroup shape -- the bytes of its traversal stacks -- and on
// the device -- its LDS per workgroup -- arrives as arguments.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bvh_build.h"
#include "prim_runs.h"

// ACCEL_K_BRUTE      uniform primitive loop (scalar loads) + shading tables staged in LDS; every table <= 32 entries,
//                    no analytic cones (device_scene.h brute_intersect CONES)
// ACCEL_K_BVH_GLOBAL stackless BVH, nodes / primitives through the vector caches (scene larger than LDS)
// ACCEL_K_BVH_LDS    stackless BVH, nodes + primitives + ids staged in LDS per workgroup
// ACCEL_K_BRUTE_BIG  uniform primitive loop, tables in global memory (brute force forced on a large scene)
enum { ACCEL_K_BRUTE = 0, ACCEL_K_BVH_GLOBAL = 1, ACCEL_K_BVH_LDS = 2, ACCEL_K_BRUTE_BIG = 3 };
#define TAB_MAX 32                // entries of a table the ACCEL_K_BRUTE variant (and k_shade) stages in LDS
#define LDS_IMAGE_NODE_BYTES 56u  // a node of the LDS image (device_scene.h TreeLds)
#define BVH_STK_OVF 30            // entries of a traversal stack's overflow in scratch memory (device_scene.h BvhStack)
#define BVH_STK_MAX (BVH_STK_OVF + 2)  // guaranteed capacity whatever n_rows is (>= 2 rows are always there)
static_assert(sizeof(HostLeafPrim) == 40 && sizeof(HostNode4) == 64, "the records the LDS-fit rule counts");

// ---- refusals -------------------------------------------------------------------------------------------------------------------
struct Refusal {
    int code = PBRT_OK;  // PBRT_E_INVALID / PBRT_E_UNSUPPORTED
    char text[192] = "";  // the whole message, as pbrt_last_error gives it
};
__attribute__((format(printf, 3, 4))) static inline int scene_refuse(Refusal *why, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(why->text, sizeof why->text, fmt, ap);
    va_end(ap);
    return why->code = code;
}
#define SCENE_RULE(cond)                                                                              \
    do {                                                                                              \
        if (!(cond)) return scene_refuse(&rq->why, PBRT_E_INVALID, "invalid argument: %s", #cond);     \
    } while (0)

// ---- the material rule ----------------------------------------------------------------------------------------------------------
// ROUGHCONDUCTOR / CONDUCTOR_FRESNEL records (include/pbrt_hip.h): alpha finite and > 0, eta and k finite and >= 0
static inline bool material_is_glossy(uint32_t type) { return type == PBRT_MAT_ROUGHCONDUCTOR || type == PBRT_MAT_CONDUCTOR_FRESNEL; }
static inline int material_rule(const pbrt_material &m, uint32_t index, Refusal *why) {
    if (!material_is_glossy(m.type)) return PBRT_OK;
    if (m.type == PBRT_MAT_ROUGHCONDUCTOR && !(std::isfinite(m.p[0]) && m.p[0] > 0.0f))
        return scene_refuse(why, PBRT_E_INVALID, "material %u: roughconductor alpha must be finite and > 0", index);
    for (int k = 1; k < 7; ++k)
        if (!(std::isfinite(m.p[k]) && m.p[k] >= 0.0f))
            return scene_refuse(why, PBRT_E_INVALID, "material %u: conductor %s must be finite and >= 0", index, k < 4 ? "eta" : "k");
    return PBRT_OK;
}

// ---- the facts ------------------------------------------------------------------------------------------------------------------
// What the driver chooses kernels by; a pbrt_scene carries them for its lifetime.
struct SceneFacts {
    int accel_kernel = ACCEL_K_BRUTE;
    uint32_t lds_bytes = 0;  // ACCEL_K_BVH_LDS: bytes of the image, rounded up to 16
    uint32_t bvh_depth = 0;  // levels of inner nodes of the BVH4
    bool curved = true;      // the scene holds spheres, cones or cylinders (else the BVH stream kernels run without their tests)
    bool cylinders = false;  // the scene holds cylinders (else the stream shading kernels run without their code)
    // a material is a ROUGHCONDUCTOR or CONDUCTOR_FRESNEL (else the bounce and the stream shading kernels run the instances
    // without their code); follows pbrt_scene_update_material through mat_types
    bool glossy = false;
    bool small_tables = false;  // brute-force scenes: everything the ACCEL_K_BRUTE variant needs holds (tables <= 32 entries, no quadrics, no vertex normals)
    std::vector<uint32_t> mat_types;
};
// the kernel variant of a brute-force scene: only ACCEL_K_BRUTE_BIG carries the cone / cylinder, the shading-normal and the
// rough / Fresnel conductor code
static inline int brute_variant(bool small_tables, bool glossy) { return small_tables && !glossy ? ACCEL_K_BRUTE : ACCEL_K_BRUTE_BIG; }
// glossy from the material types, and with it the variant of a brute-force scene: at creation and after every material update
static inline void scene_set_glossy(SceneFacts *f) {
    f->glossy = false;
    for (uint32_t t : f->mat_types) f->glossy = f->glossy || material_is_glossy(t);
    if (f->accel_kernel == ACCEL_K_BRUTE || f->accel_kernel == ACCEL_K_BRUTE_BIG) f->accel_kernel = brute_variant(f->small_tables, f->glossy);
}

// Where a built tree goes: ACCEL_K_BVH_LDS with *lds_bytes -- the image, 56 bytes per node (planes, device_scene.h TreeLds) + the
// leaf records, fits beside the traversal stacks of a 1024-thread workgroup (stack_bytes) and the kernels' small static arrays
// (1 KiB of slack) --, else ACCEL_K_BVH_GLOBAL; or -1: the traversal state cannot hold the tree -- one stack entry per level of
// inner nodes, 24-bit node indices, 27-bit leaf records (device_scene.h BvhStack).
static inline int tree_placement(size_t n_nodes, uint32_t n_prims, uint32_t depth, uint32_t lds_limit, uint32_t stack_bytes, uint32_t accel,
                                 uint32_t *lds_bytes) {
    if (depth > BVH_STK_MAX || n_nodes >= (1u << 24) - 1u || n_prims >= (1u << 27)) return -1;
    const size_t lds = n_nodes * LDS_IMAGE_NODE_BYTES + (size_t)n_prims * sizeof(HostLeafPrim);
    if (!(lds_limit && lds + stack_bytes + 1024 <= lds_limit && accel != PBRT_ACCEL_BVH_GLOBAL)) return ACCEL_K_BVH_GLOBAL;
    *lds_bytes = (uint32_t)((lds + 15) & ~size_t(15));
    return ACCEL_K_BVH_LDS;
}

// ---- the request ----------------------------------------------------------------------------------------------------------------
struct SceneRequest {
    Refusal why;
    const pbrt_scene_desc *d;
    uint32_t lds_limit, stack_bytes;
    bool want_bvh;
    // a tree whose leaf records alone exceed the LDS stays in global memory whatever its shape: the SAH constant of those trees
    bool sure_global;
    SceneFacts facts;  // (a BVH scene: accel_kernel, lds_bytes and bvh_depth once its tree is placed, scene_place)
};

// -> PBRT_OK and *rq filled, or the code of the first rule that failed, rq->why its message.  out: the caller has a place for the
// handle.  lds_limit: LDS bytes of a workgroup on the device (0: unknown); stack_bytes: see tree_placement.
static inline int scene_request(SceneRequest *rq, const pbrt_scene_desc *d, bool out, uint32_t lds_limit, uint32_t stack_bytes) {
    rq->why = Refusal{};
    SCENE_RULE(d && out);
    SCENE_RULE(d->n_prims > 0 && d->prims && d->n_materials > 0 && d->materials);
    SCENE_RULE(d->n_emitters == 0 || d->emitters);
    SCENE_RULE(d->n_light_prims == 0 || (d->light_prims && d->light_cdf));
    bool quadrics = false, curved = false, cylinders = false;
    for (uint32_t i = 0; i < d->n_prims; ++i) {
        const pbrt_prim &p = d->prims[i];
        if (p.type > PBRT_PRIM_CYLINDER) return scene_refuse(&rq->why, PBRT_E_UNSUPPORTED, "primitive %u: type %u is not supported", i, p.type);
        double c0[3], c1[3], ca[3], cb[3];
        if (p.type == PBRT_PRIM_CONE && !cone_world_frame(p, c0, ca, cb, c1))
            return scene_refuse(&rq->why, PBRT_E_INVALID, "primitive %u: cone needs an invertible, finite world -> object matrix", i);
        if (p.type == PBRT_PRIM_CYLINDER && !cylinder_world_frame(p, c0, c1, ca, cb))
            return scene_refuse(&rq->why, PBRT_E_INVALID, "primitive %u: cylinder needs an invertible, finite world -> object matrix", i);
        if (p.material >= d->n_materials) return scene_refuse(&rq->why, PBRT_E_INVALID, "primitive %u: material out of range", i);
        if (p.emitter >= 0 && (uint32_t)p.emitter >= d->n_emitters)
            return scene_refuse(&rq->why, PBRT_E_INVALID, "primitive %u: emitter out of range", i);
        quadrics = quadrics || p.type == PBRT_PRIM_CONE || p.type == PBRT_PRIM_CYLINDER;
        curved = curved || (p.type != PBRT_PRIM_TRIANGLE && p.type != PBRT_PRIM_PARALLELOGRAM);
        cylinders = cylinders || p.type == PBRT_PRIM_CYLINDER;
    }
    for (uint32_t i = 0; i < d->n_materials; ++i)
        if (int rc = material_rule(d->materials[i], i, &rq->why)) return rc;
    for (uint32_t i = 0; i < d->n_emitters; ++i) {
        const pbrt_emitter &e = d->emitters[i];
        if (e.type == PBRT_EMIT_AREA) {
            if (e.count == 0 || e.first + e.count > d->n_light_prims)
                return scene_refuse(&rq->why, PBRT_E_INVALID, "emitter %u: light primitive range out of bounds", i);
            for (uint32_t k = 0; k < e.count; ++k) {
                uint32_t pi = d->light_prims[e.first + k];
                if (pi >= d->n_prims || d->prims[pi].type == PBRT_PRIM_SPHERE || d->prims[pi].type == PBRT_PRIM_CONE ||
                    d->prims[pi].type == PBRT_PRIM_CYLINDER)
                    return scene_refuse(&rq->why, PBRT_E_UNSUPPORTED, "emitter %u: area lights need triangle/parallelogram primitives", i);
            }
        } else if (e.type != PBRT_EMIT_POINT) {
            return scene_refuse(&rq->why, PBRT_E_INVALID, "emitter %u: unknown type", i);
        }
    }
    if (d->vertex_normals)
        for (size_t i = 0; i < (size_t)d->n_prims * 9; ++i)
            if (!std::isfinite(d->vertex_normals[i])) return scene_refuse(&rq->why, PBRT_E_INVALID, "vertex_normals: entry %zu is not finite", i);
    SCENE_RULE(d->accel <= PBRT_ACCEL_BVH_GLOBAL);
    rq->d = d;
    rq->lds_limit = lds_limit;
    rq->stack_bytes = stack_bytes;
    rq->want_bvh = d->accel == PBRT_ACCEL_BVH || d->accel == PBRT_ACCEL_BVH_GLOBAL || (d->accel == PBRT_ACCEL_AUTO && d->n_prims > 32);
    rq->sure_global = !lds_limit || (size_t)d->n_prims * sizeof(HostLeafPrim) > lds_limit || d->accel == PBRT_ACCEL_BVH_GLOBAL;
    SceneFacts &f = rq->facts = SceneFacts{};
    // (only the _BIG variant carries the cone / cylinder code, and the shading-normal code)
    f.small_tables = !rq->want_bvh && d->n_prims <= TAB_MAX && d->n_materials <= TAB_MAX && d->n_emitters <= TAB_MAX && !quadrics && !d->vertex_normals;
    if (rq->want_bvh) {  // (brute-force scenes keep the defaults: their kernels carry the sphere test anyway)
        f.accel_kernel = ACCEL_K_BVH_GLOBAL;
        f.curved = curved;
        f.cylinders = cylinders;
    }
    for (uint32_t i = 0; i < d->n_materials; ++i) f.mat_types.push_back(d->materials[i].type);
    scene_set_glossy(&f);
    return PBRT_OK;
}

// ---- the host tables ------------------------------------------------------------------------------------------------------------
// Primitives that can occlude a segment between two points of the scene (DevScene::occ_prims).  A planar
// primitive is dropped when all OTHER geometry and every point emitter lie in one closed half-space of its
// plane: it then sits on the boundary of the scene's convex hull and a segment whose end points are in the
// hull cannot cross it.  Exact comparisons (>= 0 in f64 on the f32 data), so nearly-coplanar scenes just
// keep their primitives.
static inline std::vector<pbrt_prim> find_occluders(const pbrt_scene_desc *d) {
    std::vector<pbrt_prim> occ;
    for (uint32_t i = 0; i < d->n_prims; ++i) {
        const pbrt_prim &P = d->prims[i];
        bool keep = true;
        if (P.type == PBRT_PRIM_TRIANGLE || P.type == PBRT_PRIM_PARALLELOGRAM) {
            const double n[3] = {P.g[9], P.g[10], P.g[11]}, p0[3] = {P.g[0], P.g[1], P.g[2]};
            double lo = INFINITY, hi = -INFINITY;
            auto side = [&](double x, double y, double z) {
                return n[0] * (x - p0[0]) + n[1] * (y - p0[1]) + n[2] * (z - p0[2]);
            };
            auto acc = [&](double s) {
                lo = std::min(lo, s);
                hi = std::max(hi, s);
            };
            for (uint32_t j = 0; j < d->n_prims; ++j) {
                if (j == i) continue;
                const pbrt_prim &Q = d->prims[j];
                if (Q.type == PBRT_PRIM_SPHERE) {
                    double s = side(Q.g[0], Q.g[1], Q.g[2]);
                    acc(s - (double)Q.g[3]);
                    acc(s + (double)Q.g[3]);
                } else if (Q.type == PBRT_PRIM_CONE) {  // extent of the base ellipse along n, and the apex
                    double cc[3], ca[3], cb[3], cx[3];
                    cone_world_frame(Q, cc, ca, cb, cx);
                    const double s = side(cc[0], cc[1], cc[2]);
                    const double an = n[0] * ca[0] + n[1] * ca[1] + n[2] * ca[2], bn = n[0] * cb[0] + n[1] * cb[1] + n[2] * cb[2];
                    const double r = std::sqrt(an * an + bn * bn) * (1.0 + 1e-12);
                    acc(s - r);
                    acc(s + r);
                    acc(side(cx[0], cx[1], cx[2]));
                } else if (Q.type == PBRT_PRIM_CYLINDER) {  // extent of both end ellipses along n
                    double c0[3], c1[3], ca[3], cb[3];
                    cylinder_world_frame(Q, c0, c1, ca, cb);
                    const double an = n[0] * ca[0] + n[1] * ca[1] + n[2] * ca[2], bn = n[0] * cb[0] + n[1] * cb[1] + n[2] * cb[2];
                    const double r = std::sqrt(an * an + bn * bn) * (1.0 + 1e-12);
                    const double s0 = side(c0[0], c0[1], c0[2]), s1 = side(c1[0], c1[1], c1[2]);
                    acc(s0 - r);
                    acc(s0 + r);
                    acc(s1 - r);
                    acc(s1 + r);
                } else {
                    const double v0[3] = {Q.g[0], Q.g[1], Q.g[2]}, e1[3] = {Q.g[3], Q.g[4], Q.g[5]}, e2[3] = {Q.g[6], Q.g[7], Q.g[8]};
                    acc(side(v0[0], v0[1], v0[2]));
                    acc(side(v0[0] + e1[0], v0[1] + e1[1], v0[2] + e1[2]));
                    acc(side(v0[0] + e2[0], v0[1] + e2[1], v0[2] + e2[2]));
                    if (Q.type == PBRT_PRIM_PARALLELOGRAM)
                        acc(side(v0[0] + e1[0] + e2[0], v0[1] + e1[1] + e2[1], v0[2] + e1[2] + e2[2]));
                }
            }
            for (uint32_t e = 0; e < d->n_emitters; ++e)
                if (d->emitters[e].type == PBRT_EMIT_POINT)
                    acc(side(d->emitters[e].pos[0], d->emitters[e].pos[1], d->emitters[e].pos[2]));
            if (lo >= 0.0 || hi <= 0.0) keep = false;
            // a scene lit by ONE single-primitive area light: every shadow segment ends (1 - ShadowEpsilon)
            // short of that primitive's plane, so the light itself never occludes
            if (d->n_emitters == 1 && d->emitters[0].type == PBRT_EMIT_AREA && d->emitters[0].count == 1 &&
                d->light_prims[d->emitters[0].first] == i)
                keep = false;
        }
        if (keep) occ.push_back(P);
    }
    return occ;
}

// Everything a scene uploads beside the caller's own arrays, in host vectors.  Brute-force scenes: the occluder list and both
// lists cut into runs of one primitive class, in list order (prim_runs.h; brute_intersect walks them run by run); prim_ord /
// occ_ord: the counts of an ordered scene -- BOTH lists class-ordered (the occluders are a sub-sequence of the primitives, checked
// all the same) --, else 0.  BVH scenes: the BVH4 with its depth and the leaf records in leaf order.
struct SceneTables {
    std::vector<pbrt_prim> occ;
    std::vector<uint32_t> runs, occ_runs;
    uint32_t prim_ord = 0, occ_ord = 0;
    HostBvh4 b4;
    std::vector<HostLeafPrim> leaves;
};
static inline void scene_tables(const SceneRequest &rq, SceneTables *t) {
    const pbrt_scene_desc *d = rq.d;
    if (!rq.want_bvh) {
        t->occ = find_occluders(d);
        t->runs = cut_prim_runs(d->prims, d->n_prims);
        t->occ_runs = cut_prim_runs(t->occ.data(), t->occ.size());
        uint32_t cnt[3], occ_cnt[3];
        if (prim_runs_ordered(t->runs, cnt) && prim_runs_ordered(t->occ_runs, occ_cnt) && prim_ord_pack(cnt) && prim_ord_pack(occ_cnt)) {
            t->prim_ord = prim_ord_pack(cnt);
            t->occ_ord = prim_ord_pack(occ_cnt);
        }
        return;
    }
    HostBvh bvh;
    build_bvh(d->prims, d->n_prims, &bvh, rq.sure_global ? BVH_CTRAV_GLOBAL : BVH_CTRAV);
    to_bvh4(bvh, &t->b4);
    make_leaf_prims(d->prims, bvh.order, &t->leaves);
}

// The tree of a BVH scene placed (tree_placement): the facts it decides, or the refusal.  Brute-force scenes: nothing to place.
static inline int scene_place(SceneRequest *rq, const SceneTables &t) {
    if (!rq->want_bvh) return PBRT_OK;
    SceneFacts &f = rq->facts;
    f.accel_kernel = tree_placement(t.b4.nodes.size(), rq->d->n_prims, t.b4.depth, rq->lds_limit, rq->stack_bytes, rq->d->accel, &f.lds_bytes);
    f.bvh_depth = t.b4.depth;
    if (f.accel_kernel < 0)
        return scene_refuse(&rq->why, PBRT_E_UNSUPPORTED, "BVH depth %u / %zu nodes exceed the traversal state", t.b4.depth, t.b4.nodes.size());
    return PBRT_OK;
}
