// Host-side check of csrc/workspace.h (the named device buffers of a context): the type is bound to a host allocator that hands
// the most recently freed block back first, so "the same address again" happens every time.  Built with
// -fsanitize=address,undefined by tests/test_workspace_host.py; prints one JSON line, exit status 1 if a check failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "workspace.h"

struct HostAlloc {
    struct Block {
        void *p;
        size_t cap;
    };
    static std::vector<Block> all, freed;  // every block ever made; the ones that are free, most recent last
    static int n_alloc, n_free, fail_with;  // fail_with != 0: the next alloc returns it
    static const int out_of_memory = 2;
    static int alloc(void **p, size_t bytes) {
        if (fail_with) {
            const int e = fail_with;
            fail_with = 0;
            return e;
        }
        ++n_alloc;
        if (!freed.empty() && freed.back().cap >= bytes) {
            *p = freed.back().p;
            freed.pop_back();
            return 0;
        }
        *p = malloc(bytes);
        all.push_back({*p, bytes});
        return 0;
    }
    static void free(void *p) {
        ++n_free;
        for (const Block &b : all)
            if (b.p == p) {
                freed.push_back(b);
                return;
            }
        abort();  // not one of ours
    }
    static const char *error_string(int e) { return e == out_of_memory ? "out of memory" : "other error"; }
    static size_t live() { return all.size() - freed.size(); }
};
std::vector<HostAlloc::Block> HostAlloc::all, HostAlloc::freed;
int HostAlloc::n_alloc = 0, HostAlloc::n_free = 0, HostAlloc::fail_with = 0;

using WS = Workspace<HostAlloc>;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
        }                                                                  \
    } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

int main() {
    unsetenv("PBRT_DEBUG_ALLOC_FAIL_BYTES");
    const size_t KiB = 1024, MiB = 1024 * 1024;

    // padded size: 12.5 % + 256 below 64 MiB, + 256 from there on
    CHECK(WS::padded(KiB) == 1024 + 128 + 256);
    CHECK(WS::padded(64 * MiB - 1) == (64 * MiB - 1) + (64 * MiB - 1) / 8 + 256);
    CHECK(WS::padded(64 * MiB) == 64 * MiB + 256);

    {  // the epoch rises on every path that frees; generations
        WS w;
        uint64_t seq = 1;
        CHECK(w.generation("a") == 0 && w.total() == 0 && w.bytes("a") == 0);
        void *a = w.get("a", KiB, seq);
        void *b = w.get("b", KiB, seq);
        CHECK(a && b && a != b && w.epoch() == 0);
        CHECK(w.total() == 2 * WS::padded(KiB) && w.bytes("a") == WS::padded(KiB));
        const uint64_t ga = w.generation("a"), gb = w.generation("b");
        CHECK(ga != 0 && gb != 0 && ga != gb);
        CHECK(w.get("a", KiB + 100, seq) == a && w.generation("a") == ga && w.epoch() == 0);  // fits the slack: the same allocation
        // regrow
        uint64_t e = w.epoch();
        void *a2 = w.get("a", 4 * KiB, seq);
        CHECK(a2 && w.epoch() == e + 1 && w.generation("a") != ga && w.generation("a") != 0);
        CHECK(w.generation("b") == gb);  // untouched: the same generation
        // release, and the block comes back at the same address under another generation
        const uint64_t ga2 = w.generation("a");
        e = w.epoch();
        w.release("a");
        CHECK(w.epoch() == e + 1 && w.generation("a") == 0 && w.bytes("a") == 0);
        void *a3 = w.get("a", 4 * KiB, seq);
        CHECK(a3 == a2);  // the allocator's promise: the same address again
        CHECK(w.generation("a") != ga2 && w.generation("a") != ga && w.generation("a") != 0 && w.epoch() == e + 1);
        w.release("nothing");  // absent: nothing happens
        CHECK(w.epoch() == e + 1);
        // trim: "b" was not asked for by call 2
        ++seq;
        CHECK(w.get("a", 4 * KiB, seq) == a3);
        e = w.epoch();
        w.trim(seq);
        CHECK(w.epoch() == e + 1 && w.generation("b") == 0 && w.generation("a") != 0 && w.total() == WS::padded(4 * KiB));
        // release_all
        CHECK(w.get("b", KiB, seq) != nullptr);
        e = w.epoch();
        w.release_all();
        CHECK(w.epoch() == e + 2 && w.total() == 0 && w.generation("a") == 0 && w.generation("b") == 0);
        CHECK(HostAlloc::live() == 0);
    }

    {  // trim keeps a buffer exactly when its stamp is current and its size is at most the padded size of its last request
        WS w;
        uint64_t seq = 1;
        w.get("stale", KiB, seq);
        w.get("big", 100 * KiB, seq);
        w.get("edge", 8 * KiB, seq);
        ++seq;
        w.get("fits", KiB, seq);
        w.get("big", KiB, seq);  // current, but far larger than this call needed
        CHECK(w.get("edge", 8 * KiB, seq) != nullptr);  // asked again at its size: held == padded(need), the boundary on the kept side
        const uint64_t g_fits = w.generation("fits"), g_edge = w.generation("edge");
        w.trim(seq);
        CHECK(w.generation("stale") == 0 && w.generation("big") == 0);
        CHECK(w.generation("fits") == g_fits && w.generation("edge") == g_edge);
        CHECK(w.total() == WS::padded(KiB) + WS::padded(8 * KiB));
        ++seq;
        CHECK(WS::padded(8 * KiB - 1) == WS::padded(8 * KiB) - 2);
        CHECK(w.get("edge", 8 * KiB - 1, seq) != nullptr && w.generation("edge") == g_edge);  // one byte less re-uses it ...
        w.trim(seq);
        CHECK(w.generation("edge") == 0 && w.generation("fits") == 0 && w.total() == 0);  // ... but holds 2 bytes more than its padded size: it goes
        // touch_all: what a replayed recording uses survives a trim
        w.get("x", KiB, seq);
        w.get("y", KiB, seq);
        seq += 5;
        w.touch_all(seq);
        const uint64_t e = w.epoch();
        w.trim(seq);
        CHECK(w.epoch() == e && w.generation("x") != 0 && w.generation("y") != 0);
        w.release_all();
    }

    {  // under a limit: what the current call has not stamped goes first, the buffer being requested survives
        WS w;
        uint64_t seq = 1;
        w.limit = 3 * WS::padded(16 * KiB);
        void *a = w.get("a", 16 * KiB, seq);
        void *b = w.get("b", 16 * KiB, seq);
        void *c0 = w.get("c", 16 * KiB, seq);
        CHECK(a && b && c0 && w.total() == w.limit);
        ++seq;
        CHECK(w.get("a", 16 * KiB, seq) == a);
        const uint64_t ga = w.generation("a");
        uint64_t e = w.epoch();
        void *d = w.get("d", 16 * KiB, seq);  // no room: "b" and "c" (call 1) go, "a" (this call) stays
        CHECK(d && w.epoch() == e + 2 && w.generation("b") == 0 && w.generation("c") == 0 && w.generation("a") == ga);
        CHECK(w.total() == 2 * WS::padded(16 * KiB));
        // the requested buffer itself, grown under the limit: freed and allocated again, its entry survives the eviction
        ++seq;
        e = w.epoch();
        void *a2 = w.get("a", 40 * KiB, seq);  // "a" and "d" are of call 2 now: both go ("a" as the regrow, "d" as the eviction)
        CHECK(a2 && w.epoch() == e + 2 && w.generation("a") != ga && w.generation("a") != 0 && w.generation("d") == 0);
        CHECK(w.total() == WS::padded(40 * KiB) && w.bytes("a") == WS::padded(40 * KiB));
        // room cannot be made: everything held is of this call
        const size_t held = w.total();
        const uint64_t ga2 = w.generation("a");
        e = w.epoch();
        const int allocs = HostAlloc::n_alloc;
        CHECK(w.get("e", 16 * KiB, seq) == nullptr);
        CHECK(has(w.error, "workspace limit: e wants") && w.total() == held && w.generation("e") == 0 && w.bytes("e") == 0);
        CHECK(w.generation("a") == ga2 && w.epoch() == e && HostAlloc::n_alloc == allocs);
        const std::string limit_error = w.error;

        // a simulated allocation failure leaves the same state
        w.limit = 0;
        setenv("PBRT_DEBUG_ALLOC_FAIL_BYTES", "8192", 1);
        CHECK(w.get("f", 16 * KiB, seq) == nullptr);
        CHECK(has(w.error, "hipMalloc(") && has(w.error, "for f: out of memory") && w.error != limit_error);
        CHECK(w.total() == held && w.generation("f") == 0 && w.bytes("f") == 0 && w.generation("a") == ga2 && w.epoch() == e);
        CHECK(HostAlloc::n_alloc == allocs);  // (the allocator was not asked)
        CHECK(w.get("small", KiB, seq) != nullptr);  // below the size: granted
        unsetenv("PBRT_DEBUG_ALLOC_FAIL_BYTES");
        // ... and so does a failure of the allocator itself
        HostAlloc::fail_with = 7;
        CHECK(w.get("g", 16 * KiB, seq) == nullptr && has(w.error, "for g: other error"));
        CHECK(w.total() == held + WS::padded(KiB) && w.generation("g") == 0 && w.bytes("g") == 0 && w.epoch() == e);
        CHECK(w.get("g", 16 * KiB, seq) != nullptr && w.generation("g") != 0);  // the entry is usable afterwards
        w.release_all();
    }

    {  // while the context records: a missing buffer is refused, a present one is handed out, nothing is allocated or freed
        WS w;
        const uint64_t seq = 1;
        void *a = w.get("a", KiB, seq);
        const uint64_t ga = w.generation("a");
        const int allocs = HostAlloc::n_alloc, frees = HostAlloc::n_free;
        CHECK(w.get("a", KiB, seq + 1, true) == a && w.generation("a") == ga);
        CHECK(w.get("b", KiB, seq + 1, true) == nullptr && has(w.error, "run the chain once before recording it"));
        CHECK(w.get("a", 64 * KiB, seq + 1, true) == nullptr && w.generation("a") == ga);  // too small counts as missing, and stays
        CHECK(w.epoch() == 0 && HostAlloc::n_alloc == allocs && HostAlloc::n_free == frees && w.generation("b") == 0);
        w.release_all();
    }

    CHECK(HostAlloc::live() == 0);
    for (const HostAlloc::Block &b : HostAlloc::all) free(b.p);
    printf("{\"checks\": %d, \"failures\": %d}\n", checks, failures);
    return failures ? 1 : 0;
}
