// Run tables of the brute-force primitive lists (device_scene.h brute_intersect): a list is cut into maximal runs of
// consecutive records of one class, in list order, and the device walks it run by run with one straight-line loop per class
// -- no type test per primitive.  A run is one word, count << 2 | class.  Plain host code (no HIP), so that
// tests/native/prim_runs_check.cpp can build it on its own.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/pbrt_hip.h"

#define PRIM_RUN_QUAD 0u    // PBRT_PRIM_PARALLELOGRAM
#define PRIM_RUN_TRI 1u     // PBRT_PRIM_TRIANGLE
#define PRIM_RUN_CURVED 2u  // PBRT_PRIM_SPHERE / _CONE / _CYLINDER
#define PRIM_RUN_MAX_COUNT 0x3fffffffu

static inline uint32_t prim_run_class(uint32_t type) {
    return type == PBRT_PRIM_PARALLELOGRAM ? PRIM_RUN_QUAD : type == PBRT_PRIM_TRIANGLE ? PRIM_RUN_TRI : PRIM_RUN_CURVED;
}

static inline std::vector<uint32_t> cut_prim_runs(const pbrt_prim *prims, size_t n) {
    std::vector<uint32_t> runs;
    for (size_t i = 0; i < n;) {
        const uint32_t cls = prim_run_class(prims[i].type);
        size_t j = i + 1;
        while (j < n && j - i < PRIM_RUN_MAX_COUNT && prim_run_class(prims[j].type) == cls) ++j;
        runs.push_back((uint32_t)(j - i) << 2 | cls);
        i = j;
    }
    return runs;
}

// A list is class-ordered when its table holds at most one run per class, in the order PRIM_RUN_QUAD, PRIM_RUN_TRI,
// PRIM_RUN_CURVED (classes may be absent, the list may be empty): the device then walks it as three straight-line loops over
// the counts (nq, nt, nc) and reads no table (device_scene.h brute_intersect ORDERED).  A class whose records exceed
// PRIM_RUN_MAX_COUNT is cut into two runs and so is not ordered.  cnt is written on true only.
static inline bool prim_runs_ordered(const uint32_t *runs, size_t n_runs, uint32_t cnt[3]) {
    uint32_t c[3] = {0u, 0u, 0u};
    uint32_t next = PRIM_RUN_QUAD;  // the lowest class the next run may have
    for (size_t r = 0; r < n_runs; ++r) {
        const uint32_t cls = runs[r] & 3u;
        if (cls > PRIM_RUN_CURVED || cls < next) return false;
        c[cls] = runs[r] >> 2;
        next = cls + 1u;
    }
    cnt[0] = c[0];
    cnt[1] = c[1];
    cnt[2] = c[2];
    return true;
}
static inline bool prim_runs_ordered(const std::vector<uint32_t> &runs, uint32_t cnt[3]) {
    return prim_runs_ordered(runs.data(), runs.size(), cnt);
}

// The counts of a class-ordered list as the device reads them (DevScene::prim_ord / occ_ord): PRIM_ORD_VALID | nq | nt << 10 |
// nc << 20, never 0.  0: a count does not fit its PRIM_ORD_BITS bits -- such a list keeps the table walk.
#define PRIM_ORD_BITS 10u
#define PRIM_ORD_MASK ((1u << PRIM_ORD_BITS) - 1u)
#define PRIM_ORD_VALID 0x80000000u
static inline uint32_t prim_ord_pack(const uint32_t cnt[3]) {
    if (cnt[0] > PRIM_ORD_MASK || cnt[1] > PRIM_ORD_MASK || cnt[2] > PRIM_ORD_MASK) return 0u;
    return PRIM_ORD_VALID | cnt[0] | cnt[1] << PRIM_ORD_BITS | cnt[2] << (2u * PRIM_ORD_BITS);
}
