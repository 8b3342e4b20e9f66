// workspace.h -- the named device buffers of a context (pbrt_api.hip: pbrt_ctx::work).  Host code only, nothing of HIP: the device
// allocator is a policy (pbrt_api.hip binds hipMalloc / hipFree; tests/native/workspace_check.cpp a host allocator), so every rule
// below is checked on the CPU.
//
// Buffers grow on demand and are re-used by later calls.  `limit` (0: none) caps their sum: a request that would exceed it first
// evicts what the current call has not asked for, and fails if that is not enough -- the render paths answer by taking smaller
// passes.  trim() gives back what the last call did not need.
//
// Two counters tell the caches and recordings that hang off a buffer whether it is still the one they knew:
//   epoch()          rises whenever a buffer leaves the device (every path goes through drop()), and whenever the context replaces
//                    something else a finished recording refers to (invalidate_recordings(): tables, the tap table, a caller's
//                    device buffer, a scene)
//   generation(name) a number unique per allocation, 0 while the buffer is absent: a buffer that was freed and came back, even at
//                    the same address, has another one
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

// Alloc: static int alloc(void **, size_t) (0: success), static void free(void *), static const char *error_string(int),
// static const int out_of_memory (the code of a simulated failure)
template <class Alloc>
class Workspace {
public:
    size_t limit = 0;
    uint64_t epoch() const { return epoch_; }
    void invalidate_recordings() { ++epoch_; }
    std::string error;  // why the last get() returned nullptr

    // small buffers get 12.5 % of slack (a slightly larger request re-uses them); the large ones -- path state, ray and radiance
    // records, sized by the pass -- are allocated as asked
    static size_t padded(size_t bytes) { return bytes < (size_t(64) << 20) ? bytes + bytes / 8 + 256 : bytes + 256; }

    // The buffer `name` with room for `bytes`, stamped with the call that asks; nullptr on failure (`error` says why, the entry then
    // holds no pointer).  frozen (the context's stream records): what is there is handed out, nothing is allocated.
    void *get(const char *name, size_t bytes, uint64_t call_seq, bool frozen = false) {
        Buf &b = bufs[name];
        b.need = bytes;
        b.stamp = call_seq;
        if (b.bytes >= bytes && b.p) return b.p;
        if (frozen) return fail("recording: workspace buffer %s (%zu bytes) is not there yet -- run the chain once before recording it", name, bytes);
        drop(b);
        const size_t want = padded(bytes);
        if (limit && total() + want > limit)  // make room: what this call has not asked for goes first
            for (auto it = bufs.begin(); it != bufs.end();) {
                if (it->second.stamp != call_seq && &it->second != &b) {
                    drop(it->second);
                    it = bufs.erase(it);
                } else {
                    ++it;
                }
            }
        if (limit && total() + want > limit)
            return fail("workspace limit: %s wants %zu bytes on top of %zu held, limit %zu", name, want, total(), limit);
        // PBRT_DEBUG_ALLOC_FAIL_BYTES (tests of the halve-the-pass retry): a request above this size fails the way an allocation
        // that lost the race against another allocator does.  Read per allocation: a test sets and clears it.
        const char *dbg_fail = getenv("PBRT_DEBUG_ALLOC_FAIL_BYTES");
        const int e = (dbg_fail && want > (size_t)strtoull(dbg_fail, nullptr, 0)) ? Alloc::out_of_memory : Alloc::alloc(&b.p, want);
        if (e != 0) {
            b.p = nullptr;
            return fail("hipMalloc(%zu) for %s: %s", want, name, Alloc::error_string(e));
        }
        b.bytes = want;
        b.gen = ++last_gen;
        return b.p;
    }
    void release(const char *name) {
        auto it = bufs.find(name);
        if (it == bufs.end()) return;
        drop(it->second);
        bufs.erase(it);
    }
    void release_all() {
        for (auto &kv : bufs) drop(kv.second);
        bufs.clear();
    }
    // frees every buffer the call `call_seq` did not use, and every one that is larger than that call needed
    void trim(uint64_t call_seq) {
        for (auto it = bufs.begin(); it != bufs.end();) {
            Buf &b = it->second;
            if (b.stamp != call_seq || b.bytes > padded(b.need) || !b.p) {
                drop(b);
                it = bufs.erase(it);
            } else {
                ++it;
            }
        }
    }
    size_t total() const {
        size_t t = 0;
        for (const auto &kv : bufs) t += kv.second.bytes;
        return t;
    }
    size_t bytes(const char *name) const {
        auto it = bufs.find(name);
        return it == bufs.end() ? 0 : it->second.bytes;
    }
    // a replayed recording uses what it was recorded with: a trim between launches must not take it
    void touch_all(uint64_t call_seq) {
        for (auto &kv : bufs) kv.second.stamp = call_seq;
    }
    uint64_t generation(const char *name) const {
        auto it = bufs.find(name);
        return it == bufs.end() || !it->second.p ? 0 : it->second.gen;
    }

private:
    struct Buf {
        void *p = nullptr;
        size_t bytes = 0;    // allocated
        size_t need = 0;     // what the most recent request asked for
        uint64_t stamp = 0;  // call_seq of that request
        uint64_t gen = 0;    // of this allocation
    };
    std::map<std::string, Buf> bufs;
    uint64_t last_gen = 0, epoch_ = 0;

    // the one way a buffer leaves the device
    void drop(Buf &b) {
        if (b.p) {
            Alloc::free(b.p);
            ++epoch_;
        }
        b.p = nullptr;
        b.bytes = 0;
        b.gen = 0;
    }
    template <class... Args>
    void *fail(const char *fmt, Args... args) {
        char msg[1024];
        snprintf(msg, sizeof msg, fmt, args...);
        error = msg;
        return nullptr;
    }
};
