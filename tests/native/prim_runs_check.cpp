// Host check of csrc/prim_runs.h (tests/test_prim_runs_host.py builds and runs it under the sanitizers): the run tables of the
// brute-force primitive lists tile a list in order, their counts sum to n, no two neighbouring runs share a class, and every
// run has the class of the records it covers.  Prints one JSON line: {"checks": N, "failures": M}.
#include <cstdio>
#include <vector>

#include "prim_runs.h"

static int checks = 0, failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        ++checks;                                                     \
        if (!(cond)) {                                                \
            ++failures;                                               \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);   \
        }                                                             \
    } while (0)

static std::vector<pbrt_prim> list_of(const std::vector<uint32_t> &types) {
    std::vector<pbrt_prim> v(types.size());
    for (size_t i = 0; i < types.size(); ++i) v[i].type = types[i];
    return v;
}

// the properties every table must have; returns the number of runs
static size_t check_table(const std::vector<uint32_t> &types) {
    const std::vector<pbrt_prim> prims = list_of(types);
    const std::vector<uint32_t> runs = cut_prim_runs(prims.data(), prims.size());
    size_t at = 0;
    for (size_t r = 0; r < runs.size(); ++r) {
        const uint32_t cnt = runs[r] >> 2, cls = runs[r] & 3u;
        CHECK(cnt >= 1);
        CHECK(cls <= PRIM_RUN_CURVED);
        CHECK(at + cnt <= types.size());
        for (size_t k = at; k < at + cnt && k < types.size(); ++k) CHECK(prim_run_class(types[k]) == cls);  // in order, right class
        if (r > 0) CHECK((runs[r - 1] & 3u) != cls);                                                       // maximal runs
        at += cnt;
    }
    CHECK(at == types.size());  // the counts sum to n
    return runs.size();
}

int main() {
    const uint32_t T = PBRT_PRIM_TRIANGLE, S = PBRT_PRIM_SPHERE, Q = PBRT_PRIM_PARALLELOGRAM, C = PBRT_PRIM_CONE, Y = PBRT_PRIM_CYLINDER;
    CHECK(prim_run_class(Q) == PRIM_RUN_QUAD && prim_run_class(T) == PRIM_RUN_TRI);
    CHECK(prim_run_class(S) == PRIM_RUN_CURVED && prim_run_class(C) == PRIM_RUN_CURVED && prim_run_class(Y) == PRIM_RUN_CURVED);
    // an empty list (also through a null pointer, as an empty std::vector hands out)
    CHECK(cut_prim_runs(nullptr, 0).empty());
    CHECK(check_table({}) == 0);
    // one primitive of every type
    for (uint32_t t : {T, S, Q, C, Y}) {
        CHECK(check_table({t}) == 1);
        const std::vector<pbrt_prim> one = list_of({t});
        CHECK(cut_prim_runs(one.data(), 1)[0] == (1u << 2 | prim_run_class(t)));
    }
    // all of one class
    CHECK(check_table(std::vector<uint32_t>(7, Q)) == 1);
    CHECK(check_table(std::vector<uint32_t>(7, T)) == 1);
    CHECK(check_table(std::vector<uint32_t>(7, S)) == 1);
    // strictly alternating classes: every run has length one
    {
        std::vector<uint32_t> alt;
        for (int i = 0; i < 32; ++i) alt.push_back(i % 3 == 0 ? T : i % 3 == 1 ? S : Q);
        CHECK(check_table(alt) == 32);
        CHECK(check_table({T, Q, T, Q, T}) == 5);
    }
    // a cone and a cylinder among spheres: one curved run
    CHECK(check_table({S, C, S, Y, S}) == 1);
    CHECK(check_table({Q, Q, S, C, Y, S, T}) == 3);
    {
        const std::vector<pbrt_prim> v = list_of({Q, Q, S, C, Y, S, T});
        const std::vector<uint32_t> runs = cut_prim_runs(v.data(), v.size());
        CHECK(runs.size() == 3 && runs[0] == (2u << 2 | PRIM_RUN_QUAD) && runs[1] == (4u << 2 | PRIM_RUN_CURVED) &&
              runs[2] == (1u << 2 | PRIM_RUN_TRI));
    }
    // the Cornell box: six quads and two spheres
    CHECK(check_table({Q, Q, Q, Q, Q, Q, S, S}) == 2);
    // 32 and 33 primitives (the two brute-force kernel variants), mixed and uniform
    for (size_t n : {size_t(32), size_t(33)}) {
        std::vector<uint32_t> mixed;
        for (size_t i = 0; i < n; ++i) mixed.push_back((i / 3) % 3 == 0 ? Q : (i / 3) % 3 == 1 ? S : T);
        CHECK(check_table(mixed) == (n + 2) / 3);
        CHECK(check_table(std::vector<uint32_t>(n, T)) == 1);
    }
    std::printf("{\"checks\": %d, \"failures\": %d}\n", checks, failures);
    return failures ? 1 : 0;
}
