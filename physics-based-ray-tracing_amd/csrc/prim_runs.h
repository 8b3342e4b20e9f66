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
