// Host check of the ordering predicate of csrc/prim_runs.h (tests/test_ordered_runs_host.py builds and runs it under the
// sanitizers): a list is class-ordered when its run table holds at most one run per class in the order parallelograms, triangles,
// curved records; prim_runs_ordered says so and returns the three counts, prim_ord_pack packs them into the word the device
// reads.  Prints one JSON line: {"checks": N, "failures": M}.
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

static const uint32_t T = PBRT_PRIM_TRIANGLE, S = PBRT_PRIM_SPHERE, Q = PBRT_PRIM_PARALLELOGRAM, C = PBRT_PRIM_CONE, Y = PBRT_PRIM_CYLINDER;

static std::vector<uint32_t> table_of(const std::vector<uint32_t> &types) {
    std::vector<pbrt_prim> v(types.size());
    for (size_t i = 0; i < types.size(); ++i) v[i].type = types[i];
    return cut_prim_runs(v.data(), v.size());
}

// the predicate against a restatement on the types themselves: the classes never fall along the list
static bool ordered_by_types(const std::vector<uint32_t> &types, uint32_t cnt[3]) {
    cnt[0] = cnt[1] = cnt[2] = 0;
    for (size_t i = 0; i < types.size(); ++i) {
        if (i > 0 && prim_run_class(types[i]) < prim_run_class(types[i - 1])) return false;
        ++cnt[prim_run_class(types[i])];
    }
    return true;
}

static void expect_ordered(const std::vector<uint32_t> &types, uint32_t nq, uint32_t nt, uint32_t nc) {
    const std::vector<uint32_t> runs = table_of(types);
    uint32_t cnt[3] = {77u, 77u, 77u}, ref[3];
    CHECK(prim_runs_ordered(runs, cnt));
    CHECK(cnt[0] == nq && cnt[1] == nt && cnt[2] == nc);
    CHECK(cnt[0] + cnt[1] + cnt[2] == types.size());
    CHECK(ordered_by_types(types, ref) && ref[0] == nq && ref[1] == nt && ref[2] == nc);
    CHECK(prim_runs_ordered(runs.data(), runs.size(), ref) && ref[0] == nq && ref[1] == nt && ref[2] == nc);  // the pointer form
    const uint32_t w = prim_ord_pack(cnt);
    CHECK(w != 0u && (w & PRIM_ORD_VALID));
    CHECK((w & PRIM_ORD_MASK) == nq && ((w >> PRIM_ORD_BITS) & PRIM_ORD_MASK) == nt && ((w >> (2u * PRIM_ORD_BITS)) & PRIM_ORD_MASK) == nc);
    // every sub-sequence of an ordered list is ordered (the occluder list is one): all of them for short lists, else each
    // primitive dropped in turn and every second one
    const size_t n = types.size();
    auto sub_ok = [&](const std::vector<uint32_t> &sub) {
        uint32_t c[3], r[3];
        const std::vector<uint32_t> sr = table_of(sub);
        CHECK(prim_runs_ordered(sr, c));
        CHECK(ordered_by_types(sub, r) && c[0] == r[0] && c[1] == r[1] && c[2] == r[2]);
        CHECK(c[0] <= nq && c[1] <= nt && c[2] <= nc);
    };
    if (n <= 8) {
        for (uint32_t m = 0; m < (1u << n); ++m) {
            std::vector<uint32_t> sub;
            for (size_t i = 0; i < n; ++i)
                if (m >> i & 1u) sub.push_back(types[i]);
            sub_ok(sub);
        }
    } else {
        for (size_t drop = 0; drop < n; ++drop) {
            std::vector<uint32_t> sub;
            for (size_t i = 0; i < n; ++i)
                if (i != drop) sub.push_back(types[i]);
            sub_ok(sub);
        }
        for (size_t first = 0; first < 2; ++first) {
            std::vector<uint32_t> sub;
            for (size_t i = first; i < n; i += 2) sub.push_back(types[i]);
            sub_ok(sub);
        }
    }
}

static void expect_not_ordered(const std::vector<uint32_t> &types) {
    const std::vector<uint32_t> runs = table_of(types);
    uint32_t cnt[3] = {77u, 78u, 79u}, ref[3];
    CHECK(!prim_runs_ordered(runs, cnt));
    CHECK(cnt[0] == 77u && cnt[1] == 78u && cnt[2] == 79u);  // written on true only
    CHECK(!ordered_by_types(types, ref));
}

static std::vector<uint32_t> qts(size_t nq, size_t nt, size_t nc) {
    std::vector<uint32_t> v(nq, Q);
    v.insert(v.end(), nt, T);
    v.insert(v.end(), nc, S);
    return v;
}

int main() {
    // ordered: the empty list (also through a null table), single primitives, every pair and triple of classes in order
    {
        uint32_t cnt[3] = {1u, 1u, 1u};
        CHECK(prim_runs_ordered(nullptr, 0, cnt) && cnt[0] == 0 && cnt[1] == 0 && cnt[2] == 0);
        CHECK(prim_ord_pack(cnt) == PRIM_ORD_VALID);  // an empty ordered list is not "not ordered"
    }
    expect_ordered({}, 0, 0, 0);
    expect_ordered({Q}, 1, 0, 0);
    expect_ordered({T}, 0, 1, 0);
    expect_ordered({S}, 0, 0, 1);
    expect_ordered({Q, S}, 1, 0, 1);
    expect_ordered({Q, T, S}, 1, 1, 1);
    expect_ordered({T, S}, 0, 1, 1);
    expect_ordered({Q, T}, 1, 1, 0);
    expect_ordered({Q, Q, Q, Q, Q, Q, S, S}, 6, 0, 2);  // the Cornell box
    expect_ordered({Q, Q, Q, S, S}, 3, 0, 2);
    expect_ordered({T, T, S}, 0, 2, 1);
    // a cone and a cylinder inside the curved run
    expect_ordered({Q, Q, S, C, S}, 2, 0, 3);
    expect_ordered({Q, T, C, Y, S}, 1, 1, 3);
    expect_ordered({C}, 0, 0, 1);
    // 32 and 33 primitives (the two brute-force kernel variants)
    expect_ordered(qts(11, 11, 10), 11, 11, 10);
    expect_ordered(qts(11, 11, 11), 11, 11, 11);
    expect_ordered(qts(32, 0, 0), 32, 0, 0);
    expect_ordered(qts(0, 0, 33), 0, 0, 33);
    expect_ordered(qts(30, 0, 2), 30, 0, 2);
    // not ordered
    expect_not_ordered({S, Q});
    expect_not_ordered({Q, S, Q});
    expect_not_ordered({T, Q});
    expect_not_ordered({T, S, Q, T, S});
    expect_not_ordered({S, T});
    expect_not_ordered({Q, T, S, C, T});
    expect_not_ordered({Q, S, T, S});
    {
        std::vector<uint32_t> alt;
        for (int i = 0; i < 33; ++i) alt.push_back(i % 2 ? Q : S);
        expect_not_ordered(alt);
    }
    // hand-made tables: a class twice in a row (what cut_prim_runs makes of more than PRIM_RUN_MAX_COUNT records), a class
    // value that is none
    {
        uint32_t cnt[3];
        const uint32_t twice[2] = {PRIM_RUN_MAX_COUNT << 2 | PRIM_RUN_QUAD, 1u << 2 | PRIM_RUN_QUAD};
        CHECK(!prim_runs_ordered(twice, 2, cnt));
        const uint32_t bad[1] = {1u << 2 | 3u};
        CHECK(!prim_runs_ordered(bad, 1, cnt));
        const uint32_t big[1] = {PRIM_RUN_MAX_COUNT << 2 | PRIM_RUN_CURVED};
        CHECK(prim_runs_ordered(big, 1, cnt) && cnt[2] == PRIM_RUN_MAX_COUNT);
        CHECK(prim_ord_pack(cnt) == 0u);  // does not fit the packed word: the table walk
    }
    // the packed word at its limits
    {
        const uint32_t fits[3] = {PRIM_ORD_MASK, PRIM_ORD_MASK, PRIM_ORD_MASK};
        const uint32_t w = prim_ord_pack(fits);
        CHECK(w == (PRIM_ORD_VALID | 0x3fffffffu));
        for (int k = 0; k < 3; ++k) {
            uint32_t over[3] = {1u, 2u, 3u};
            over[k] = PRIM_ORD_MASK + 1u;
            CHECK(prim_ord_pack(over) == 0u);
        }
    }
    std::printf("{\"checks\": %d, \"failures\": %d}\n", checks, failures);
    return failures ? 1 : 0;
}
