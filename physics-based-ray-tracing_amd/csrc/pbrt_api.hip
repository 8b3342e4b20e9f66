// pbrt_api.hip -- host side of libpbrt_hip.so: the C-ABI of include/pbrt_hip.h.
// One pbrt_ctx per device (HIP stream, grow-only workspace in HBM, last-error string); scenes are
// uploaded once and stay resident; every entry point is synchronous on return.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>
#include <string>
#include <tuple>
#include <vector>

#include "scene_request.h"
#include "bf_request.h"
#include "us_request.h"
#include "kernels_us.h"
#include "kernels_wavefront.h"
#include "kernels_us_wavefront.h"
#include "kernels_beamform.h"
#ifdef PBRT_DIAG
#include "kernels_diag.h"  // the kernels only the diagnostic build launches
#endif
#include "stage_layout.h"
#include "workspace.h"

static std::string g_ctxless_error;

// the device allocator of a context's workspace (workspace.h)
struct HipAlloc {
    static const int out_of_memory = hipErrorOutOfMemory;
    static int alloc(void **p, size_t bytes) {
        const hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) (void)hipGetLastError();
        return e;
    }
    static void free(void *p) { (void)hipFree(p); }
    static const char *error_string(int e) { return hipGetErrorString((hipError_t)e); }
};

// the context's pinned host page: partial sums of the ultrasound counters (written by k_us_reduce_stats itself), then the guard words
#define PIN_GUARD_OFFSET ((2 + MAX_DEPTH_STATS) * REDUCE_SLICES * 8)
#define PIN_BYTES (PIN_GUARD_OFFSET + 4096)

struct pbrt_ctx {
    int device = 0;
    int n_cu = 256;  // compute units (MI355X: 256); read from the device properties
    hipStream_t stream = nullptr;
    hipStream_t st_trace = nullptr, st_shade = nullptr;  // BVH scenes, PBRT_WF_SPLIT: streams with CU masks (wf_split_streams)
    uint32_t split_s = 0;
    std::vector<hipEvent_t> sync_ev;
    std::string err;
    pbrt_stats stats{};
    // Workspace (workspace.h): named device buffers that grow on demand and are re-used by later calls.  work.limit (0: none) caps
    // their sum -- PBRT_WORKSPACE_LIMIT_BYTES at pbrt_ctx_create, pbrt_ctx_set_workspace_limit later; a request that would exceed it
    // fails with PBRT_E_NOMEM and the render paths answer by taking smaller passes -- and pbrt_ctx_trim gives back what the last call
    // did not need (a caller that shares the device with another allocator, e.g. torch beside the renderer as in USMain.py:5).
    Workspace<HipAlloc> work;
    uint64_t call_seq = 0;  // bumped by every entry point that takes workspace
    std::vector<hipEvent_t> ev_pool;
    // An acquisition that was queued without waiting (pbrt_us_acquire_queue_dev, ABI 5): what us_finish needs to turn the counters
    // the device leaves in the pinned page into pbrt_stats once the stream has drained.  Every entry point that waits for the
    // stream or starts other work on the context finishes it first (ctx_settle).
    struct PendingAcq {
        bool active = false, streams = false, tab0 = false;
        bool scaled = true;  // the normalisation pass over the channel buffer ran (not at one path per ray)
        bool timed = true;  // false: replayed from a recording (no event pairs; kernel_ms / bounce_ms are 0)
        size_t n_ev = 0;
        uint32_t passes = 0, launches = 0;
        uint64_t samples = 0, nchan = 0;
    } pend;
    // one page of pinned host memory: the statistics and guard words of a call are copied here (a copy to pageable memory blocks
    // the host until it is done; to pinned memory it is queued like a kernel)
    void *pinned = nullptr;
    unsigned long long *pin_stats() { return (unsigned long long *)pinned; }              // [2 + MAX_DEPTH_STATS][REDUCE_SLICES] partial sums
    uint32_t *pin_guard() { return (uint32_t *)((char *)pinned + PIN_GUARD_OFFSET); }      // [WF_GUARD_WORDS]
    // the ultrasound counters (workspace "us_stats") as the last acquisition left them: k_us_reduce_stats zeroes what it reads, so a
    // call that finds the same allocation (its generation; 0: not clean) and the same size skips the fill command
    uint64_t us_rows_gen = 0;
    size_t us_rows_bytes = 0;
    // the small tables of the last acquisition (transmit delays, primary directions, element positions) as uploaded into the
    // allocation us_tab_gen of workspace "us_tables": the reference's loop calls the acquisition 51 times with the same ones
    // (USMain.py:260,279-283), three host-to-device copies each
    std::vector<float> us_tab_host;
    uint64_t us_tab_gen = 0;
    // image formation (f-1): event pairs per step when profiling is on (pbrt_ctx_set_profiling), read by pbrt_get_image_stats
    bool profiling = false;
    hipEvent_t img_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    uint32_t img_mask = 0;
    uint64_t img_das_bytes = 0;
    size_t env_lds_attr = 0;
    uint32_t env_taps_n = 0;  // column length the context's tap table (workspace "env_taps") was made for ...
    uint64_t env_taps_gen = 0;  // ... in this allocation of it
    uint64_t wf_guard_gen = 0;  // the allocation of workspace "wf_guard" that was cleared
    // the keep words of the camera tiles (workspace "tile_keep") as the last render of a brute-force scene left them: a render of the
    // same scene with the same camera and region that finds the same allocation (its generation; 0: none) skips k_tile_keep -- a
    // progressive render calls with nothing but the sample offset changed, and the kernel is 20 us of a 6 ms Cornell box step
    struct TileKeepKey {
        uint64_t gen = 0, scene = 0;
        pbrt_camera cam{};
        uint32_t rx0 = 0, ry0 = 0, rw = 0, rh = 0;
        bool operator==(const TileKeepKey &o) const {
            return gen == o.gen && scene == o.scene && memcmp(&cam, &o.cam, sizeof cam) == 0 && rx0 == o.rx0 && ry0 == o.ry0 && rw == o.rw && rh == o.rh;
        }
    } tile_keep_key;
    // what pbrt_ctx_tile_keep reports: whether the LAST radiance render carried a table (the key outlives a later render without
    // one), and how often k_tile_keep has been launched
    bool tile_keep_last = false;
    const uint32_t *tile_keep_words = nullptr;  // that render's table: good while the workspace buffer is allocation tile_keep_key.gen
    uint64_t tile_keep_builds = 0;
    bool img_event(int i) { return img_ev[i] || hipEventCreate(&img_ev[i]) == hipSuccess; }
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint32_t lds_limit = 0;
    // A recording of the queued chain (pbrt_ctx_record_begin .. pbrt_ctx_record_end; replayed by pbrt_graph_launch): while it is
    // open the context's stream captures instead of running, nothing may wait for it, allocate or upload.  work.epoch() counts the
    // events that make a finished recording stale: memory it may refer to freed or replaced, other acquisition tables uploaded,
    // the envelope's tap table made for another column length.
    bool recording = false, rec_failed = false;
    std::string rec_msg;

    int fail(int code, const char *fmt, ...) {
        char buf[1024];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        if (recording && !rec_failed) {  // the first error inside a recording: pbrt_ctx_record_end reports it again and makes no graph
            rec_failed = true;
            rec_msg = buf;
        }
        return code;
    }
    // an entry point that may not run while the stream records: the same, but the recording stays good
    int refuse(const char *what) {
        err = std::string("a recording is open on this context (pbrt_ctx_record_begin): ") + what;
        return PBRT_E_INVALID;
    }
    // returns nullptr on failure (err set; the caller reports PBRT_E_NOMEM with this message)
    void *buf(const char *name, size_t bytes) {
        void *p = work.get(name, bytes, call_seq, recording);
        if (!p) fail(PBRT_E_NOMEM, "%s", work.error.c_str());
        return p;
    }
    hipEvent_t event(size_t i) {
        while (ev_pool.size() <= i) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            ev_pool.push_back(e);
        }
        return ev_pool[i];
    }
};

struct pbrt_scene : SceneFacts {  // (scene_request.h: accel_kernel, lds_bytes, bvh_depth, curved, cylinders, glossy, small_tables, mat_types)
    pbrt_ctx *ctx = nullptr;
    DevScene ds{};
    std::vector<void *> allocs;
    pbrt_material *d_mats = nullptr;
    uint32_t n_mats = 0;
    // fuse plan learnt from the path survival of the last render of this scene (brute-force kernels; 0: none yet)
    uint32_t plan_hint = 0;
    bool plan_hint_valid = false;
    uint64_t serial = 0;  // unique per scene of the process (never 0): what a context remembers a scene by (pbrt_ctx::tile_keep_key)
};

#define HIPCHK(ctx, call)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return (ctx)->fail(PBRT_E_DEVICE, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)
#define NEED(ctx, cond)                                                        \
    do {                                                                       \
        if (!(cond)) return (ctx)->fail(PBRT_E_INVALID, "invalid argument: %s", #cond); \
    } while (0)
// the material rule (scene_request.h) as an entry point reports it
#define MATERIAL_RULE(ctx, m, index)                                                                    \
    do {                                                                                                \
        Refusal why_;                                                                                   \
        if (int rc_ = material_rule(m, index, &why_)) return (ctx)->fail(rc_, "%s", why_.text);         \
    } while (0)

// entry points that wait, copy from host memory or free: not while the context's stream records (pbrt_ctx_record_begin)
#define NOT_RECORDING(ctx)                                                                                                   \
    do {                                                                                                                     \
        if ((ctx)->recording) return (ctx)->refuse((std::string(__func__) + " cannot run").c_str());                         \
    } while (0)

// finishes an acquisition that was queued without waiting (pbrt_us_acquire_queue_dev): waits for the stream, checks the guard words,
// fills pbrt_stats.  Called first by every entry point that waits for the stream or starts other work on the context.
static int us_finish(pbrt_ctx *c);
static inline int ctx_settle(pbrt_ctx *c) {
    // (every entry point that waits for the stream or starts work of its own comes through here: none of them may run while the
    // stream records -- a wait would invalidate the capture)
    if (c->recording) return c->refuse("only the queueing entry points may be called");
    return c->pend.active ? us_finish(c) : PBRT_OK;
}

template <typename T>
static int upload(pbrt_scene *s, const T *src, size_t n, const T **dst) {
    void *p = nullptr;
    size_t bytes = std::max<size_t>(n * sizeof(T), 16);
    HIPCHK(s->ctx, hipMalloc(&p, bytes));
    s->allocs.push_back(p);
    if (n) HIPCHK(s->ctx, hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    *dst = static_cast<const T *>(p);
    return PBRT_OK;
}


// Runtime flags as template arguments: with_flags(f, a, b, ...) calls the generic lambda f with one std::true_type / std::false_type
// per flag and returns what f returns.  Every kernel family has ONE selector built on it (bounce_kernel, trace_kernel, ...), which
// both its launch site and the site that sets its LDS attribute call; f names exactly the instances that exist.
template <class F>
static auto with_flags(F f) { return f(); }
template <class F, class... Bs>
static auto with_flags(F f, bool b, Bs... rest) {
    auto bind = [&](auto c) { return with_flags([&](auto... cs) { return f(c, cs...); }, rest...); };
    return b ? bind(std::true_type{}) : bind(std::false_type{});
}
// the limit of dynamic LDS of the kernel a selector returned
template <class K>
static hipError_t set_max_lds(K kernel, size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
using RadKern = void (*)(RadArgs);
using PathKern = void (*)(PathArgs);
using WfKern = void (*)(WfArgs);
using UsKern = void (*)(UsArgs);
using UsWfKern = void (*)(UsWfArgs);
using UsFirstKern = void (*)(UsArgs, uint32_t, float4 *, float4 *);
using RayIntersectKern = void (*)(DevScene, uint32_t, const float *, const float *, const float *, float *, uint32_t *, float *, float *);
using RayTestKern = void (*)(DevScene, uint32_t, const float *, const float *, const float *, uint8_t *);

extern "C" {

int pbrt_abi_version(void) { return PBRT_ABI_VERSION; }

int pbrt_ctx_create(int device, pbrt_ctx **out) {
    if (!out) {
        g_ctxless_error = "pbrt_ctx_create: out is NULL";
        return PBRT_E_INVALID;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        g_ctxless_error = std::string("no HIP device visible: ") + hipGetErrorString(e) +
                          " (the ray-transport hot path has no CPU fallback)";
        return PBRT_E_DEVICE;
    }
    if (device < 0 || device >= n) {
        g_ctxless_error = "device index out of range";
        return PBRT_E_INVALID;
    }
    pbrt_ctx *c = new pbrt_ctx();
    c->device = device;
#ifdef PBRT_CU_MASK_PROBE  // diagnostic builds: run on a subset of the CUs (PBRT_CU_MASK = even | odd | low | pairs)
    auto masked_stream = [&](hipStream_t *st) -> hipError_t {
        const char *m = getenv("PBRT_CU_MASK");
        if (!m) return hipStreamCreate(st);
        uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t b = 0; b < 256; ++b) {
            bool on = !strcmp(m, "even") ? (b & 1u) == 0 : !strcmp(m, "odd") ? (b & 1u) == 1 : !strcmp(m, "low") ? b < 128
                      : !strcmp(m, "altcu") ? ((b >> 5) & 1u) == 0 : !strcmp(m, "altse") ? ((b >> 3) & 1u) == 0 : !strcmp(m, "altcu2") ? ((b >> 6) & 1u) == 0 : !strcmp(m, "pairs") ? (b & 2u) == 0 : true;
            if (on) mask[b >> 5] |= 1u << (b & 31u);
        }
        return hipExtStreamCreateWithCUMask(st, 8, mask);
    };
    if ((e = hipSetDevice(device)) != hipSuccess || (e = masked_stream(&c->stream)) != hipSuccess ||
#else
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreate(&c->stream)) != hipSuccess ||
#endif
        (e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess) {
        g_ctxless_error = std::string("device init: ") + hipGetErrorString(e);
        delete c;
        return PBRT_E_DEVICE;
    }
    if ((e = hipHostMalloc(&c->pinned, PIN_BYTES, hipHostMallocDefault)) != hipSuccess) {
        g_ctxless_error = std::string("hipHostMalloc: ") + hipGetErrorString(e);
        (void)hipStreamDestroy(c->stream);
        delete c;
        return PBRT_E_NOMEM;
    }
    std::memset(c->pinned, 0, PIN_BYTES);
    if (const char *lim = getenv("PBRT_WORKSPACE_LIMIT_BYTES")) c->work.limit = (size_t)strtoull(lim, nullptr, 0);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        c->lds_limit = (uint32_t)prop.sharedMemPerBlock;
        if (prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
    }
    *out = c;
    return PBRT_OK;
}

int pbrt_ctx_destroy(pbrt_ctx *c) {
    if (!c) return PBRT_OK;
    (void)hipSetDevice(c->device);
    if (c->recording) {  // an open recording: close the capture and drop it
        hipGraph_t g = nullptr;
        if (hipStreamEndCapture(c->stream, &g) == hipSuccess && g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        c->recording = false;
        c->pend.active = false;
    }
    (void)ctx_settle(c);
    (void)hipStreamSynchronize(c->stream);
    if (c->st_trace) (void)hipStreamSynchronize(c->st_trace);
    if (c->st_shade) (void)hipStreamSynchronize(c->st_shade);
    c->work.release_all();
    if (c->pinned) (void)hipHostFree(c->pinned);
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (auto e : c->sync_ev) (void)hipEventDestroy(e);
    for (auto e : c->img_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->st_trace) (void)hipStreamDestroy(c->st_trace);
    if (c->st_shade) (void)hipStreamDestroy(c->st_shade);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return PBRT_OK;
}

const char *pbrt_last_error(pbrt_ctx *c) { return c ? c->err.c_str() : g_ctxless_error.c_str(); }

int pbrt_ctx_set_workspace_limit(pbrt_ctx *c, uint64_t bytes) {
    if (!c) return PBRT_E_INVALID;
    if (int rc = ctx_settle(c)) return rc;
    c->work.limit = (size_t)bytes;
    if (bytes && c->work.total() > bytes) {  // a limit below what the context holds: everything goes back (calls are synchronous, nothing is in use)
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->work.release_all();
        c->stats.workspace_bytes = 0;
    }
    return PBRT_OK;
}

// frees every workspace buffer the most recent call did not use, and every one that is larger than that call needed
int pbrt_ctx_trim(pbrt_ctx *c, uint64_t *held_after) {
    if (!c) return PBRT_E_INVALID;
    if (int rc = ctx_settle(c)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->work.trim(c->call_seq);
    c->stats.workspace_bytes = c->work.total();
    if (held_after) *held_after = c->stats.workspace_bytes;
    return PBRT_OK;
}

int pbrt_get_stats(pbrt_ctx *c, pbrt_stats *out) {
    if (!c || !out) return PBRT_E_INVALID;
    if (int rc = ctx_settle(c)) return rc;  // (a queued acquisition: its counters arrive now)
    *out = c->stats;
    return PBRT_OK;
}

// the keep table of the last radiance render (render_tile_keep): read back for tests and diagnosis, launches nothing
int pbrt_ctx_tile_keep(pbrt_ctx *c, pbrt_tile_keep_info *info, uint32_t *words, uint32_t capacity) {
    if (!c) return PBRT_E_INVALID;
    NEED(c, info && (words || capacity == 0));
    if (int rc = ctx_settle(c)) return rc;
    *info = pbrt_tile_keep_info{};
    info->builds = c->tile_keep_builds;
    if (!c->tile_keep_last) return PBRT_OK;
    const pbrt_ctx::TileKeepKey &key = c->tile_keep_key;
    if (key.gen == 0 || c->work.generation("tile_keep") != key.gen)
        return c->fail(PBRT_E_INVALID, "the keep table of the last render has left the workspace (pbrt_ctx_trim or the workspace limit after another call)");
    info->n_blocks = (uint32_t)((uint64_t)key.rw * key.rh / 64);
    info->rx0 = key.rx0;
    info->ry0 = key.ry0;
    info->rw = key.rw;
    info->rh = key.rh;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t n = std::min(info->n_blocks, capacity);
    if (n) HIPCHK(c, hipMemcpy(words, c->tile_keep_words, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PBRT_OK;
}

}  // extern "C"

// ---- pbrt_scene_create: check -> host tables -> placement -> upload -> publish ----------------------------------------------------
// What creation decides on the host -- the rules, the accelerator and its kernel variant, the occluder list, the run tables, the tree
// and where it goes -- is scene_request.h; every refusal but a failed device call comes before the first allocation.
namespace {
struct SceneCall {
    pbrt_ctx *c;
    const pbrt_scene_desc *d;
    pbrt_scene **out;
    SceneRequest rq;          // scene_check; scene_placed finishes its facts
    SceneTables tab;          // scene_tables (scene_request.h)
    pbrt_scene *s = nullptr;  // scene_upload
};
}  // namespace

static int scene_check(SceneCall &q) {
    if (scene_request(&q.rq, q.d, q.out != nullptr, q.c->lds_limit, BVH_STK_DW(SEG_BVH) * 4)) return q.c->fail(q.rq.why.code, "%s", q.rq.why.text);
    return PBRT_OK;
}

static int scene_placed(SceneCall &q) {
    static_assert(sizeof(HostLeafPrim) == sizeof(DevLeafPrim) && sizeof(DevLeafPrim) == 40, "leaf record layout");
    static_assert(sizeof(HostNode4) == sizeof(DevNode4) && sizeof(DevNode4) == 64, "node layout");
    if (scene_place(&q.rq, q.tab)) return q.c->fail(q.rq.why.code, "%s", q.rq.why.text);
    return PBRT_OK;
}

// one allocation and one copy per table, in the order they always had; a failure leaves what was allocated in q.s->allocs
static int scene_upload(SceneCall &q) {
    const pbrt_scene_desc *d = q.d;
    const SceneTables &t = q.tab;
    HIPCHK(q.c, hipSetDevice(q.c->device));
    pbrt_scene *s = q.s = new pbrt_scene();
    s->ctx = q.c;
    DevScene &ds = s->ds;
    int rc = upload(s, d->prims, d->n_prims, &ds.prims_by_id);
    if (!rc) rc = upload(s, d->materials, d->n_materials, &ds.mats);
    if (!rc) rc = upload(s, d->emitters, d->n_emitters, &ds.emitters);
    if (!rc) rc = upload(s, d->light_prims, d->n_light_prims, &ds.light_prims);
    if (!rc) rc = upload(s, d->light_cdf, d->n_light_prims, &ds.light_cdf);
    if (!rc && q.rq.want_bvh) rc = upload(s, reinterpret_cast<const DevLeafPrim *>(t.leaves.data()), t.leaves.size(), &ds.lprims);
    if (!rc && d->vertex_normals) rc = upload(s, d->vertex_normals, (size_t)d->n_prims * 9, &ds.vnormals);
    if (!rc && q.rq.want_bvh) rc = upload(s, reinterpret_cast<const DevNode4 *>(t.b4.nodes.data()), t.b4.nodes.size(), &ds.nodes);
    if (!rc && !q.rq.want_bvh) rc = upload(s, t.occ.data(), t.occ.size(), &ds.occ_prims);
    if (!rc && !q.rq.want_bvh) rc = upload(s, t.runs.data(), t.runs.size(), &ds.prim_runs);
    if (!rc && !q.rq.want_bvh) rc = upload(s, t.occ_runs.data(), t.occ_runs.size(), &ds.occ_runs);
    ds.prims = ds.prims_by_id;  // Hit::slot is the caller's index
    ds.n_prims = d->n_prims;
    ds.n_mats = d->n_materials;
    ds.n_emitters = d->n_emitters;
    ds.n_light_prims = d->n_light_prims;
    ds.n_nodes = (uint32_t)t.b4.nodes.size();
    ds.n_occ = (uint32_t)t.occ.size();
    ds.n_prim_runs = (uint32_t)t.runs.size();
    ds.n_occ_runs = (uint32_t)t.occ_runs.size();
    ds.prim_ord = t.prim_ord;
    ds.occ_ord = t.occ_ord;
    return rc;
}

// A scene that was never handed out: nothing queued and no recording can refer to its memory, so there is no acquisition to settle,
// no stream to wait for and no recording to mark stale (pbrt_scene_destroy does all three for a scene a caller has seen).
static int scene_discard(pbrt_scene *s, int rc) {
    for (void *p : s->allocs) (void)hipFree(p);
    delete s;
    return rc;
}

static void scene_publish(SceneCall &q) {
    static std::atomic<uint64_t> scene_serial{0};
    pbrt_scene *s = q.s;
    static_cast<SceneFacts &>(*s) = q.rq.facts;
    s->serial = ++scene_serial;
    s->d_mats = const_cast<pbrt_material *>(s->ds.mats);
    s->n_mats = q.d->n_materials;
    *q.out = s;
}

extern "C" {

int pbrt_scene_create(pbrt_ctx *c, const pbrt_scene_desc *d, pbrt_scene **out) {
    if (!c) return PBRT_E_INVALID;
    if (d && out) NOT_RECORDING(c);  // (behind the null rule, which scene_check reports)
    SceneCall q{c, d, out};
    int rc;
    if ((rc = scene_check(q)) != 0) return rc;
    scene_tables(q.rq, &q.tab);
    if ((rc = scene_placed(q)) != 0) return rc;
    if ((rc = scene_upload(q)) != 0) return q.s ? scene_discard(q.s, rc) : rc;
    scene_publish(q);
    return PBRT_OK;
}

int pbrt_scene_update_material(pbrt_scene *s, uint32_t index, const pbrt_material *m) {
    if (!s) return PBRT_E_INVALID;
    pbrt_ctx *c = s->ctx;
    NEED(c, m && index < s->n_mats);
    NOT_RECORDING(c);  // (a recorded copy would replay the bytes of THIS call's host block)
    MATERIAL_RULE(c, *m, index);
    HIPCHK(c, hipSetDevice(c->device));
    // in the order of the context's stream: behind an acquisition that is still queued, ahead of the next one (the 32 bytes are
    // staged before the call returns)
    HIPCHK(c, hipMemcpyAsync(s->d_mats + index, m, sizeof *m, hipMemcpyHostToDevice, c->stream));
    s->mat_types[index] = m->type;
    scene_set_glossy(s);  // glossy and the brute-force variant again, as creation derived them: the launches queued from now on
    return PBRT_OK;
}

int pbrt_scene_destroy(pbrt_scene *s) {
    if (!s) return PBRT_OK;
    NOT_RECORDING(s->ctx);
    (void)hipSetDevice(s->ctx->device);
    (void)ctx_settle(s->ctx);
    (void)hipStreamSynchronize(s->ctx->stream);  // queued work may still read the scene
    s->ctx->work.invalidate_recordings();
    for (void *p : s->allocs) (void)hipFree(p);
    delete s;
    return PBRT_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// environment switches
// ------------------------------------------------------------------------------------------------
// Every environment variable the library reads (INTEGRATION.md has the same table):
//
//   variable                      selects                                                                    read
//   PBRT_WORKSPACE_LIMIT_BYTES    cap of the context's workspace (pbrt_ctx_set_workspace_limit later)         pbrt_ctx_create
//   PBRT_DEBUG_ALLOC_FAIL_BYTES   test hook: workspace requests above this size fail like a lost hipMalloc    per allocation (workspace.h)
//   PBRT_WF_PACKET                0: camera rays of BVH scenes through k_trace, not k_trace_primary (A/B)     once per process
//   PBRT_WF_SPLIT                 s[,parts]: k_trace and k_shade on disjoint CUs through two masked streams   once per process
//   PBRT_US_GENERIC_KERNEL        1: the k_us_bounce instance that reads the quirks at run time              per call (us_impl)
//   PBRT_US_EMIT_FUSED            0: emitter rays through k_us_emit_init and the later-bounce instance         per call (us_impl)
//   PBRT_US_EMIT_PERMUTE          0: workgroup b walks region b; k > 1: another stride of the permutation     per call (us_impl)
//   PBRT_ENV_GENERAL              1: every column length through k_hilbert_env                                per call (pbrt_envelope*)
//   diagnostic build (-DPBRT_DIAG) only, read in diag_driver.h and not part of Switches:
//   PBRT_PAIR_MERGE               k: k_chain_pair with merge bounce k instead of the k_bounce chain           per call (diag_selected)
//   PBRT_US_FUSED_BVH             1: BVH scenes through the fused ultrasound bounce, not the streams          per call (diag_us_fused_bvh)
//   -DPBRT_CU_MASK_PROBE only:
//   PBRT_CU_MASK                  even | odd | low | pairs | ...: the CUs the context's stream runs on        pbrt_ctx_create
//
// "per call": read_switches() at the top of the driver call, so a caller (a test) may change them between two calls of one process.
struct Switches {
    bool wf_packet = true;
    uint32_t wf_split_s = 0, wf_split_parts = 1;  // s = 0: off
    bool us_generic_kernel = false, us_emit_fused = true, env_general = false;
    int us_emit_permute = 1;  // 0: off, 1: the library's stride, > 1: that stride
};
static Switches read_switches() {
    static const Switches once = [] {  // the two that hold for the process
        Switches w;
        if (const char *e = getenv("PBRT_WF_PACKET")) w.wf_packet = atoi(e) != 0;
        unsigned s_ = 0, p_ = 2;
        const char *e = getenv("PBRT_WF_SPLIT");
        if (e && sscanf(e, "%u%*[,:]%u", &s_, &p_) >= 1 && s_ >= 1 && s_ <= 7) {
            w.wf_split_s = s_;
            w.wf_split_parts = std::max(2u, std::min(p_, 8u));
        }
        return w;
    }();
    Switches w = once;
    auto flag = [](const char *name, bool unset) {
        const char *e = getenv(name);
        return e ? atoi(e) != 0 : unset;
    };
    w.us_generic_kernel = flag("PBRT_US_GENERIC_KERNEL", false);
    w.us_emit_fused = flag("PBRT_US_EMIT_FUSED", true);
    w.env_general = flag("PBRT_ENV_GENERAL", false);
    if (const char *e = getenv("PBRT_US_EMIT_PERMUTE")) w.us_emit_permute = atoi(e);
    return w;
}

// ------------------------------------------------------------------------------------------------
// radiance mode driver
// ------------------------------------------------------------------------------------------------
// What the driver decides on the host -- the argument rules, the rendered region, the shape of a pass, the fuse plan, the pass
// schedule, the stream grids, the byte models -- is render_request.h; the stages below talk to the device.
// The fused bounce kernel of a launch that walks nb bounces (>= 2: the multi-bounce variants of the brute-force kernels,
// kernels_radiance.h; a.nb = nb).  Glossy brute-force scenes have instances of their own.  nullptr: BVH scenes run k_trace /
// k_shade (wf_bounces); their fused bounce (PBRT_FILM_NO_HIT_POOL) and k_walk exist in the diagnostic build only (diag_driver.h).
// ordered: the launch's lists are class-ordered (RadArgs::sc.prim_ord != 0: the scene's, unless PBRT_FILM_NO_ORDERED_WALK took it back):
// ACCEL_K_BRUTE then runs the instances that walk them without the run tables; the _BIG / glossy instances keep the table walk.
static RadKern bounce_kernel(const pbrt_scene *s, bool first, uint32_t nb, bool ordered) {
    const bool two = nb >= 2;
    switch (s->accel_kernel) {
        case ACCEL_K_BRUTE:
            return with_flags([](auto F, auto O, auto N) -> RadKern {
                return &k_bounce<F(), O() ? ACCEL_K_BRUTE_ORDERED : ACCEL_K_BRUTE, N() ? 2 : 1>; }, first, ordered, two);
        case ACCEL_K_BRUTE_BIG:
            return with_flags([](auto F, auto G, auto N) -> RadKern {
                return &k_bounce<F(), G() ? ACCEL_K_BRUTE_GLOSSY : ACCEL_K_BRUTE_BIG, N() ? 2 : 1>; }, first, s->glossy, two);
        default:
            return nullptr;
    }
}
static int launch_bounce(pbrt_scene *s, const RadArgs &a, uint32_t nseg, bool first, uint32_t nb = 1) {
    const RadKern k = bounce_kernel(s, first, nb, a.sc.prim_ord != 0u);
    if (!k) return s->ctx->fail(PBRT_E_UNSUPPORTED, "launch_bounce: no fused bounce kernel for accelerator %d in this build", s->accel_kernel);
    hipLaunchKernelGGL(k, dim3(nseg), dim3(seg_threads(s->accel_kernel)), 0u, s->ctx->stream, a);
    return PBRT_OK;
}
// k_path (kernels_radiance.h): the launch of a pass of camera paths whose every bounce one launch walks, for ACCEL_K_BRUTE scenes
// (none of which is glossy: those are _BIG).  nullptr: the pass takes k_bounce.
static PathKern path_kernel(const pbrt_scene *s, bool ordered) {
    if (s->accel_kernel != ACCEL_K_BRUTE || s->glossy) return nullptr;
    return with_flags([](auto O) -> PathKern { return &k_path<O() ? ACCEL_K_BRUTE_ORDERED : ACCEL_K_BRUTE, PATH_THREADS>; }, ordered);
}
// The launch over the nseg regions of a pass: path_groups_per_region workgroups each, one statistics row per workgroup (the rows a
// render of such a scene has, render_launch).  No path survives it: the regions' survivor counts are cleared as k_bounce leaves them.
static int launch_path(pbrt_scene *s, PathKern k, const RadArgs &a, uint32_t nseg) {
    pbrt_ctx *c = s->ctx;
    const uint32_t groups = nseg * path_groups_per_region();
    NEED(c, a.key_mode == 0 && a.depth == 0 && a.max_depth <= MAX_CHAIN && a.stat_stride >= groups && (uint64_t)groups * PATH_THREADS <= a.cap);
    HIPCHK(c, hipMemsetAsync(a.seg_out, 0, (size_t)nseg * 4, c->stream));
    hipLaunchKernelGGL(k, dim3(groups), dim3(PATH_THREADS), 0u, c->stream, path_args(a));
    return PBRT_OK;
}

// The fused ultrasound bounce.  q: us_kernel_quirks; tab: first-bounce tables both there (1), both absent (0), else -1.
// ACCEL_K_BRUTE with a compiled-in quirk set (the kernels of BASELINE config 3, both readings, and of the reference's own loop)
// has its table mode compiled in too: -1 on later bounces, 0 for emitter rays (never any tables).  Everything else reads both at
// run time.  nullptr: BVH scenes run k_trace / k_us_shade (us_wf_pass); their fused bounce (PBRT_US_FUSED_BVH=1, no emitter rays)
// exists in the diagnostic build only (diag_driver.h; launch_us takes it from there).
// convex (PBRT_US_ARRAY_CONVEX, D18): the curved array has the generic instances only (quirks and tables read at run time).
static UsKern us_bounce_kernel(const pbrt_scene *s, bool first, bool emit, uint32_t q, int tab, bool convex = false) {
    if (!first) tab = -1;
    if (convex) {
        q = US_Q_RUNTIME;
        tab = -1;
    }
    switch (s->accel_kernel) {
        case ACCEL_K_BRUTE:
            if (q != US_Q_RUNTIME && (tab >= 0 || !first))
                return with_flags([](auto F, auto E, auto C, auto T) -> UsKern {
                    return &k_us_bounce<F(), ACCEL_K_BRUTE, E(), C() ? PBRT_USQ_REFERENCE : (PBRT_USQ_REFERENCE | PBRT_USQ_NO_CARRIER),
                                        !F() ? -1 : (!E() && T()) ? 1 : 0>; }, first, emit, q == PBRT_USQ_REFERENCE, tab == 1);
            return with_flags([](auto F, auto E, auto X) -> UsKern {
                return &k_us_bounce<F(), ACCEL_K_BRUTE, E(), US_Q_RUNTIME, -1, X()>; }, first, emit, convex);
        case ACCEL_K_BRUTE_BIG:
            return with_flags([](auto F, auto E, auto X) -> UsKern {
                return &k_us_bounce<F(), ACCEL_K_BRUTE_BIG, E(), US_Q_RUNTIME, -1, X()>; }, first, emit, convex);
        default:
            return nullptr;
    }
}


// ---- BVH scenes: intersection and shading as separate streams (kernels_wavefront.h) -------------------------------------------
struct WfPlan {
    bool packet = true;      // camera rays: one tree walk per 64-path tile (k_trace_primary); PBRT_WF_PACKET=0: k_trace (A/B)
    uint32_t grid_deep = 2;  // workgroups per CU from bounce 2 on (few rays: a resident round of larger shares; ring 8 / 2 / 1: 139.7 / 137.1 / 134.9 ms)
    uint32_t threads = 1024, rows = 2, grid_mult = 8;  // grid: ring 1024^2 x 64: 2 / 4 / 8 / 16 workgroups per CU -> 27.6 / 21.3 / 20.4 / 21.3 ms
    size_t lds = 0;
    uint32_t split_s = 0, split_parts = 1;  // PBRT_WF_SPLIT (wf_bounces); s = 0: off
};
// Workgroup shape of k_trace (render_request.h wf_shape) and the switches of the call
static WfPlan wf_plan(const pbrt_scene *s, const Switches &sw) {
    WfPlan p;
    const WfShape w = wf_shape(s->ctx->lds_limit, s->accel_kernel == ACCEL_K_BVH_LDS ? s->lds_bytes : 0u, s->bvh_depth, sw.wf_packet);
    p.threads = w.threads;
    p.rows = w.rows;
    p.lds = w.lds;
    p.packet = w.packet;
    p.split_s = sw.wf_split_s;
    p.split_parts = sw.wf_split_parts;
    return p;
}
// The intersection kernel of a bounce with its workgroup size and dynamic LDS: camera rays as packets (k_trace_primary), else
// k_trace.  Template arguments: <first bounce,> tree in LDS / in global memory, scene with curved primitives.
struct TraceLaunch {
    WfKern kernel;
    uint32_t threads;
    size_t lds;
};
static TraceLaunch trace_kernel(const pbrt_scene *s, const WfPlan &p, bool first) {
    const bool lds = s->accel_kernel == ACCEL_K_BVH_LDS;
    if (first && p.packet) {
        auto primary = [](auto L, auto C) -> WfKern { return &k_trace_primary<L() ? ACCEL_K_BVH_LDS : ACCEL_K_BVH_GLOBAL, C()>; };
        return {with_flags(primary, lds, s->curved), 1024u, lds ? s->lds_bytes : 0u};
    }
    auto trace = [](auto F, auto L, auto C) -> WfKern { return &k_trace<F(), L() ? ACCEL_K_BVH_LDS : ACCEL_K_BVH_GLOBAL, C()>; };
    return {with_flags(trace, first, lds, s->curved), p.threads, p.lds};
}
// trees in LDS: the LDS limit of the kernels this scene's bounces launch (first bounce, later bounces)
static int wf_set_attr(pbrt_scene *s, const WfPlan &p) {
    if (s->accel_kernel != ACCEL_K_BVH_LDS) return PBRT_OK;
    for (bool first : {true, false}) {
        const TraceLaunch t = trace_kernel(s, p, first);
        HIPCHK(s->ctx, set_max_lds(t.kernel, t.lds));
    }
    return PBRT_OK;
}
// the context's guard words (k_trace's turn guard): allocated and cleared once, cleared again after a trip
static uint32_t *wf_guard(pbrt_ctx *c) {
    uint32_t *g = (uint32_t *)c->buf("wf_guard", WF_GUARD_WORDS * 4);
    const uint64_t gen = c->work.generation("wf_guard");
    if (g && gen != c->wf_guard_gen) {
        if (hipMemsetAsync(g, 0, WF_GUARD_WORDS * 4, c->stream) != hipSuccess) return nullptr;
        c->wf_guard_gen = gen;
    }
    return g;
}
#define WF_BYTES_PER_PATH (2 * WF_STATE_Q * 16 + 4 + 2 * 64 + 16)  // two state sets, hit index, two shadow sets, Lhome
// the buffers whose size follows the pass: given back before a retry with half the paths in flight (render_impl, us_impl)
static void release_pass_buffers(pbrt_ctx *c) {
    for (const char *nm : {"wf_stateA", "wf_stateB", "wf_shadowA", "wf_shadowB", "wf_hit_id", "Lhome", "stateA", "stateB"}) c->work.release(nm);
}
struct WfBufs {
    float4 *stA, *stB, *shA, *shB;
    uint32_t *hit_id, *segA, *segB, *nshA, *nshB;
};
static bool wf_alloc(pbrt_ctx *c, uint32_t cap, uint32_t nreg, WfBufs *b) {
    b->stA = (float4 *)c->buf("wf_stateA", (size_t)cap * WF_STATE_Q * 16);
    b->stB = (float4 *)c->buf("wf_stateB", (size_t)cap * WF_STATE_Q * 16);
    b->hit_id = (uint32_t *)c->buf("wf_hit_id", (size_t)cap * 4);
    b->shA = (float4 *)c->buf("wf_shadowA", (size_t)cap * 64);
    b->shB = (float4 *)c->buf("wf_shadowB", (size_t)cap * 64);
    b->segA = (uint32_t *)c->buf("wf_segA", (size_t)nreg * 4);
    b->segB = (uint32_t *)c->buf("wf_segB", (size_t)nreg * 4);
    b->nshA = (uint32_t *)c->buf("wf_nshA", (size_t)nreg * 4);
    b->nshB = (uint32_t *)c->buf("wf_nshB", (size_t)nreg * 4);
    return b->stA && b->stB && b->hit_id && b->shA && b->shB && b->segA && b->segB && b->nshA && b->nshB;
}
// the buffers of a pass in their in / out roles: state, shadow rays, live counters, shadow-ray counters; flip() after every bounce
struct WfPing {
    float4 *in, *out, *shi, *sho;
    uint32_t *sin, *sout, *ni, *no;
    explicit WfPing(const WfBufs &b) : in(b.stA), out(b.stB), shi(b.shA), sho(b.shB), sin(b.segA), sout(b.segB), ni(b.nshA), no(b.nshB) {}
    void flip() {
        std::swap(in, out);
        std::swap(shi, sho);
        std::swap(sin, sout);
        std::swap(ni, no);
    }
    // the stream members of a launch's arguments (WfArgs, UsWfArgs) in the current roles, over n regions from region0 on
    template <class A>
    void bind(A &a, const WfBufs &b, bool have_shadows, uint32_t region0, uint32_t n_regions) const {
        a.st_in = in;
        a.st_out = out;
        a.hit_id = b.hit_id;
        a.shd_in = shi;
        a.shd_out = sho;
        a.seg_in = sin;
        a.seg_out = sout;
        a.nsh_in = have_shadows ? ni : nullptr;
        a.nsh_out = no;
        a.region0 = region0;
        a.n_regions = n_regions;
    }
};
// the tree and stack members of a k_trace launch, and the guard words (false: out of memory)
static bool wf_tree_args(pbrt_scene *s, const WfPlan &p, WfArgs *a) {
    a->lds_bytes = s->accel_kernel == ACCEL_K_BVH_LDS ? s->lds_bytes : 0u;
    a->stk_rows = p.rows;
    a->stk_shift = 0;
    while ((1u << a->stk_shift) < p.threads) ++a->stk_shift;
    return (a->guard = wf_guard(s->ctx)) != nullptr;
}
// BVH scenes, opt-in (PBRT_WF_SPLIT=s[,parts]): the CUs are split between the two kernels of a bounce.  k_trace is bound by
// instruction issue and k_shade by HBM, but run side by side on the same CUs they only trade wave slots (round 3: +2.8 %).  Here
// two streams carry CU masks -- s CUs of every shader engine (32 s of the 256) run k_shade, the others k_trace -- and a pass is
// cut into `parts` sets of regions that go through the two streams one phase apart: trace(part, d) -> shade(part, d) ->
// trace(part, d + 1), with trace of one part running beside shade of another.  Regions share nothing (their own slots of every
// buffer, their own statistics rows), so any order renders the same film.
static int wf_split_streams(pbrt_ctx *c, uint32_t s_cus) {
    if (c->st_trace && c->split_s == s_cus) return PBRT_OK;
    if (c->st_trace) {
        (void)hipStreamDestroy(c->st_trace);
        (void)hipStreamDestroy(c->st_shade);
        c->st_trace = c->st_shade = nullptr;
    }
    // bit b of a CU mask: XCC b % 8, shader engine (b >> 3) % 4, CU b >> 5 (tools/cu_mask_probe.hip): the s highest CUs of every
    // shader engine of every XCD shade, so both kernels have CUs on every XCD (their L2s) and every shader engine
    uint32_t mt[8] = {0}, ms[8] = {0};
    for (uint32_t bit = 0; bit < 256; ++bit) ((bit >> 5) >= 8u - s_cus ? ms : mt)[bit >> 5] |= 1u << (bit & 31u);
    HIPCHK(c, hipExtStreamCreateWithCUMask(&c->st_trace, 8, mt));
    HIPCHK(c, hipExtStreamCreateWithCUMask(&c->st_shade, 8, ms));
    c->split_s = s_cus;
    return PBRT_OK;
}

// one k_trace / k_trace_primary launch over a.n_regions regions
static void wf_launch_trace(pbrt_scene *s, const WfArgs &a, const WfPlan &p, uint32_t G, bool first, hipStream_t st) {
    const TraceLaunch t = trace_kernel(s, p, first);
    hipLaunchKernelGGL(t.kernel, dim3(G), dim3(t.threads), t.lds, st, a);
}

// k_shade with or without the cylinder code (the instance without it is the one every other scene runs), or with the rough /
// Fresnel conductor code on top of it (GLOSSY, always with CYL); the small shading tables in LDS when they fit (wf_tables_lds)
static WfKern shade_kernel(const pbrt_scene *s, bool first) {
    const bool tabs = s->ds.n_mats <= TAB_MAX && s->ds.n_emitters <= TAB_MAX && s->ds.n_light_prims <= TAB_MAX;
    if (s->glossy) return with_flags([](auto F, auto T) -> WfKern { return &k_shade<F(), T(), true, true>; }, first, tabs);
    return with_flags([](auto F, auto T, auto C) -> WfKern { return &k_shade<F(), T(), C()>; }, first, tabs, s->cylinders);
}

// Unbounded depth (Mitsuba max_depth = -1): the live paths of a pass, summed over its n counters (one per region or wave of it)
// once the stream has drained.  The caller decides when to poll and what a total of 0 ends.
static int live_paths(pbrt_ctx *c, const uint32_t *d_counts, uint32_t n, uint64_t *live) {
    std::vector<uint32_t> cnt(n);
    HIPCHK(c, hipMemcpyAsync(cnt.data(), d_counts, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *live = 0;
    for (uint32_t v : cnt) *live += v;
    return PBRT_OK;
}

// When to poll: a pass of more than 32 bounces looks whenever its bounces pass a multiple of 8 (from depth `before` to `after`).
static int poll_live(pbrt_ctx *c, uint32_t max_depth, uint32_t before, uint32_t after, const uint32_t *d_counts, uint32_t n, bool *dead) {
    *dead = false;
    if (max_depth <= 32 || (after >> 3) == (before >> 3)) return PBRT_OK;
    uint64_t live;
    if (int rc = live_paths(c, d_counts, n, &live)) return rc;
    *dead = live == 0;
    return PBRT_OK;
}

// The bounces of one pass.  camera: depth 0 generates its rays from the film keys (else the rays are in b.stA / b.segA).
// Returns the number of launches through *launches.
static int wf_bounces(pbrt_scene *s, WfArgs a, const WfBufs &b, const WfPlan &p, uint32_t nreg, bool camera, uint32_t *launches) {
    pbrt_ctx *c = s->ctx;
    if (!wf_tree_args(s, p, &a)) return PBRT_E_NOMEM;
    a.vis_q = 4;
    const bool split = p.split_s != 0 && c->n_cu == 256 && nreg >= 64u * p.split_parts && a.max_depth <= 32;
    const uint32_t parts = split ? p.split_parts : 1u;
    if (split) {
        int rc = wf_split_streams(c, p.split_s);
        if (rc) return rc;
    }
    const uint32_t cu_trace = split ? 256u - 32u * p.split_s : (uint32_t)c->n_cu;
    hipStream_t st_t = split ? c->st_trace : c->stream, st_s = split ? c->st_shade : c->stream;
    uint32_t reg0[8], regn[8];
    for (uint32_t h = 0; h < parts; ++h) wf_part(nreg, parts, h, &reg0[h], &regn[h]);
    // events of the split pipeline: [part][0] = its last k_trace, [part][1] = its last k_shade (a wait captures the record that
    // precedes it, so one event per part and kind serves every depth)
    if (split)
        while (c->sync_ev.size() < 2u * parts + 1u) {
            hipEvent_t e;
            HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            c->sync_ev.push_back(e);
        }
    WfPing pp(b);
    auto fill = [&](uint32_t depth, bool have_shadows, uint32_t h) {
        a.depth = depth;
        pp.bind(a, b, have_shadows, reg0[h], regn[h]);
    };
    auto trace = [&](uint32_t depth, bool first, bool have_shadows, uint32_t h) {
        fill(depth, have_shadows, h);
        const uint32_t nr = regn[h];
        const uint32_t mult = depth >= 2 ? p.grid_deep : p.grid_mult;
        wf_launch_trace(s, a, p, wf_trace_grid(nr, mult, cu_trace, WF_KMAX), first, st_t);
        ++*launches;
    };
    auto shade = [&](uint32_t depth, bool first, bool have_shadows, uint32_t h) {
        fill(depth, have_shadows, h);
        hipLaunchKernelGGL(shade_kernel(s, first), dim3(regn[h]), dim3(WF_SHADE_THREADS), 0, st_s, a);
        ++*launches;
    };
    if (split) {  // both masked streams start behind whatever the context's stream holds
        hipEvent_t e0 = c->sync_ev[2u * parts];
        HIPCHK(c, hipEventRecord(e0, c->stream));
        HIPCHK(c, hipStreamWaitEvent(st_t, e0, 0));
        HIPCHK(c, hipStreamWaitEvent(st_s, e0, 0));
    }
    bool flush = false;
    for (uint32_t depth = 0; depth < a.max_depth; ++depth) {
        const bool first = camera && depth == 0;
        for (uint32_t h = 0; h < parts; ++h) {
            if (split && depth > 0) HIPCHK(c, hipStreamWaitEvent(st_t, c->sync_ev[2u * h + 1u], 0));  // shade(h, depth - 1)
            trace(depth, first, depth > 0, h);
            if (split) HIPCHK(c, hipEventRecord(c->sync_ev[2u * h], st_t));
        }
        for (uint32_t h = 0; h < parts; ++h) {
            if (split) HIPCHK(c, hipStreamWaitEvent(st_s, c->sync_ev[2u * h], 0));  // trace(h, depth)
            shade(depth, first, depth > 0, h);
            if (split) HIPCHK(c, hipEventRecord(c->sync_ev[2u * h + 1u], st_s));
        }
        pp.flip();
        HIPCHK(c, hipGetLastError());
        bool dead;  // (never split: one stream)
        if (int rc = poll_live(c, a.max_depth, depth, depth + 1, pp.sin, nreg, &dead)) return rc;
        if (dead) {
            flush = depth + 1 < a.max_depth;  // the last bounce may have left shadow rays behind
            a.depth = depth + 1;
            break;
        }
    }
    if (flush) {
        const uint32_t d = a.depth;
        trace(d, false, true, 0);
        shade(d, false, true, 0);
        pp.flip();
        HIPCHK(c, hipGetLastError());
    }
    if (split)  // the context's stream goes on (film gather) when every part has been shaded
        for (uint32_t h = 0; h < parts; ++h) HIPCHK(c, hipStreamWaitEvent(c->stream, c->sync_ev[2u * h + 1u], 0));
    return PBRT_OK;
}
// Default paths in flight per pass of the trace / shade streams (render_request.h stream_default_pass_paths) from what the device
// has free now and what this context already holds for the buffers of a pass
static uint64_t wf_default_pass_paths(pbrt_ctx *c) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    size_t held = 0;
    for (const char *nm : {"wf_stateA", "wf_stateB", "wf_shadowA", "wf_shadowB", "wf_hit_id", "Lhome"}) held += c->work.bytes(nm);
    return stream_default_pass_paths(free_b, total_b, held, c->work.limit, c->work.total(), WF_BYTES_PER_PATH);
}

// The guard words of the context come back with the statistics of a call (wf_guard_fetch queues the copy on the call's stream,
// wf_check_guard looks at them once the stream has drained): did a wave of k_trace run into its turn guard?
static int wf_guard_fetch(pbrt_ctx *c, uint32_t *host) {
    uint32_t *g = wf_guard(c);
    if (!g) return PBRT_E_NOMEM;
    HIPCHK(c, hipMemcpyAsync(host, g, WF_GUARD_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    return PBRT_OK;
}
static int wf_check_guard(pbrt_ctx *c, const uint32_t *g) {
#ifdef PBRT_WF_PROBE
    {
        unsigned long long pr[8];
        std::memcpy(pr, g + 32, sizeof pr);
        fprintf(stderr, "WF_PROBE walk trips %llu lanes %llu (%.3f) holding a leaf %.3f idle %.3f | leaf trips %llu lanes %llu (%.3f) | main trips %llu rays %llu busy lanes per trip %.1f\n",
                pr[0], pr[1], pr[0] ? pr[1] / (64.0 * pr[0]) : 0.0, pr[0] ? pr[7] / (64.0 * pr[0]) : 0.0,
                pr[0] ? 1.0 - (pr[1] + pr[7]) / (64.0 * pr[0]) : 0.0, pr[2], pr[3], pr[2] ? pr[3] / (64.0 * pr[2]) : 0.0, pr[4], pr[5],
                pr[4] ? (double)pr[6] / pr[4] : 0.0);
        (void)hipMemsetAsync(wf_guard(c) + 32, 0, 64, c->stream);
    }
#endif
    if (g[0] == 0 && g[WF_GUARD_REHIT] == 0) return PBRT_OK;
    HIPCHK(c, hipMemsetAsync(wf_guard(c), 0, WF_GUARD_WORDS * 4, c->stream));
    if (g[0] == 0)
        return c->fail(PBRT_E_DEVICE, "k_shade / k_us_shade: %u hit(s) reported by k_trace were not reproduced by the repeated primitive "
                                      "test (the two must share their arithmetic and their build flags); the result is not valid",
                       g[WF_GUARD_REHIT]);
    float f[7];
    std::memcpy(f, g + 21, sizeof f);
    return c->fail(PBRT_E_DEVICE,
                   "k_trace: %u wave(s) hit the turn guard (block %u wave %u: busy %u walking %u queue_empty %u total %u q_in %u "
                   "depth 0x%x K %u | lane: cur %x sp %u tos %x rslot %x rows %x %x ovf %x %x o %g %g %g d %g %g %g best %g n_rows %u "
                   "shift %u nodes %u)",
                   g[0], g[1], g[2], g[3], g[4], g[6], g[7], g[8], g[10], g[11], g[12], g[13], g[14], g[15], g[16], g[17],
                   g[19], g[20], f[0], f[1], f[2], f[3], f[4], f[5], f[6], g[28], g[29], g[30]);
}

// ---- pass handling of the radiance and ultrasound drivers ---------------------------------------------------------------------
// ONE event pair per pass around its bounce launches (a pair per launch costs ~8 us of queue bubbles each): pair i is
// ev_pool[2 i], ev_pool[2 i + 1].  While an acquisition is recorded (timed = false) the events are taken but not recorded: event
// pairs recorded into a graph cannot be read back.  (Internal linkage: the library exports the ABI of include/pbrt_hip.h.)
namespace {
struct PassTimer {
    pbrt_ctx *c;
    bool timed = true;
    size_t n_ev = 0;  // events taken so far (call_stats reads the pairs; us_finish through PendingAcq::n_ev)
    hipEvent_t e1 = nullptr;
    int begin() {
        e1 = c->event(n_ev + 1);
        hipEvent_t e0 = c->event(n_ev);
        if (!e0 || !e1) return c->fail(PBRT_E_DEVICE, "hipEventCreate failed");
        n_ev += 2;
        if (timed) HIPCHK(c, hipEventRecord(e0, c->stream));
        return PBRT_OK;
    }
    int end() {
        if (timed) HIPCHK(c, hipEventRecord(e1, c->stream));
        return PBRT_OK;
    }
};
}  // namespace
// The pbrt_stats members both drivers fill alike, from the reduced rows (segments, shadow rays, live paths per depth) and the events
// of the call (timed: kernel_ms = c->ev0 .. c->ev1, bounce_ms = the pass pairs among the first n_ev events of the pool, added up;
// else 0 ms).  The driver adds what is its own to c->stats.
static int call_stats(pbrt_ctx *c, const unsigned long long *hstats, uint64_t samples, uint32_t launches, uint32_t passes, bool timed,
                      size_t n_ev) {
    float ms = 0.0f;
    double bounce_ms = 0.0;
    if (timed) {
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        for (size_t i = 0; i + 1 < n_ev; i += 2) {
            float t = 0.0f;
            HIPCHK(c, hipEventElapsedTime(&t, c->ev_pool[i], c->ev_pool[i + 1]));
            bounce_ms += t;
        }
    }
    pbrt_stats &S = c->stats;
    S = pbrt_stats{};
    S.samples = samples;
    S.segments = hstats[0];
    S.shadow_rays = hstats[1];
    S.kernel_ms = ms;
    S.bounce_ms = bounce_ms;
    S.bounce_launches = launches;
    S.passes = passes;
    for (int d = 0; d < 16; ++d) S.live[d] = hstats[2 + d];
    S.workspace_bytes = c->work.total();
    return PBRT_OK;
}

#ifndef US_PASS_PATHS
// an acquisition's paths in flight per pass.  Config 3 (268 M paths), one launch per bounce: 8 / 16 / 32 / 64 Mi -> 13.1 / 12.7 / 13.0 /
// 13.2 ms; with all bounces of a pass in one launch the survivors are re-read while still cached and smaller passes
// win: 2 / 4 / 6 / 8 / 12 / 16 / 32 / 64 Mi -> 13.1 / 9.8 / 8.4 / 8.1 / 8.2 / 8.5 / 9.0 / 8.7 ms.  Later in round 2 (Mitsuba's
// shading frame: 1.96 segments per path; three workgroups per CU): 4 / 8 / 16 / 32 Mi -> 13.26 / 11.89 / 11.61 / 12.20 ms
#define US_PASS_PATHS (16u << 20)
#endif
// Sizing a pass (render_request.h pass_shape: the shape, pass_addressing: what the kernels can address, pass_halve: the next size).
// The free-memory figure behind a default pass_paths is a snapshot (torch or another process may allocate between the query and the
// hipMalloc): alloc(ps) returns PBRT_E_NOMEM when the pass buffers do not fit, and then they go back, the pass is halved and tried
// again -- the result does not depend on the pass size (global path keys).  A caller-fixed pass size (fixed) gives up at once.  What
// did fit goes back too when even the smallest pass does not (the caller may be about to give the memory to someone else); the
// message of the failed request stands.  Any other code from alloc is returned as is.  rows: dwords per slot of the fused kernels'
// state.
#define RULE_TEXT(c, why) (c)->fail(PBRT_E_INVALID, "invalid argument: %s", why)
// one pass of a fixed size: its shape, held to what the kernels can address
static int one_pass(pbrt_ctx *c, uint64_t pass_paths, uint32_t per_call, uint64_t unit, uint32_t region, bool equal, bool streams,
                    uint32_t rows, PassShape *ps) {
    if (const char *why = pass_shape(ps, pass_paths, per_call, unit, region, equal)) return RULE_TEXT(c, why);
    if (const char *why = pass_addressing(ps->cap, streams, rows, WF_DEAD)) return RULE_TEXT(c, why);
    return PBRT_OK;
}
template <typename Alloc>
static int size_pass(pbrt_ctx *c, uint64_t pass_paths, bool fixed, uint32_t per_call, uint64_t unit, uint32_t region, bool equal,
                     bool streams, uint32_t rows, Alloc alloc, PassShape *ps) {
    for (;;) {
        if (int rc = one_pass(c, pass_paths, per_call, unit, region, equal, streams, rows, ps)) return rc;
        const int rc = alloc(*ps);
        if (rc != PBRT_E_NOMEM) return rc;
        release_pass_buffers(c);
        if (!pass_halve(&pass_paths, fixed, *ps, unit)) return PBRT_E_NOMEM;
    }
}
// Default paths in flight per pass: the trace / shade streams size it from the free device memory (wf_default_pass_paths); the fused
// kernels take `paths`, halved under a workspace limit until bytes_per_path of each fit it
static uint64_t default_pass_paths(pbrt_ctx *c, bool streams, uint64_t paths, uint32_t bytes_per_path) {
    return streams ? wf_default_pass_paths(c) : fused_default_pass_paths(paths, bytes_per_path, c->work.limit);
}

// self-check of a fast divisor (film_key.h make_fastdiv) against `/` at the probe values of its caller
static bool fastdiv_exact(const FastDiv &fd, uint32_t d, std::initializer_list<uint32_t> probes) {
    for (uint32_t n : probes)
        if (udiv_fast(n, fd) != n / d) return false;
    return true;
}

// ---- radiance passes ----------------------------------------------------------------------------------------------------------
// The members WfArgs shares with RadArgs (scene, camera, radiance records, statistics rows, paths, depth, seed, path keys): the
// radiance drivers fill a RadArgs, and the trace / shade streams of BVH scenes take these from it.
static WfArgs wf_args(const RadArgs &a) {
    WfArgs w{};
    w.sc = a.sc;
    w.cam = a.cam;
    w.Lhome = a.Lhome;
    w.stats = a.stats;
    w.stat_stride = a.stat_stride;
    w.cap = a.cap;
    w.n_paths = a.n_paths;
    w.max_depth = a.max_depth;
    w.rr_depth = a.rr_depth;
    w.seed = a.seed;
    w.key_mode = a.key_mode;
    w.key = a.key;
    w.index_offset = a.index_offset;
    w.sample_index = a.sample_index;
    return w;
}
// Film accumulation of one pass (k_film_accum, or the tiled gather of the tent and Gaussian filters)
static void film_accum(pbrt_ctx *c, const FilmArgs &fa) {
    hipStream_t st = c->stream;
    if (fa.filter == PBRT_FILTER_BOX) {
        hipLaunchKernelGGL(k_film_accum, dim3(div_up((uint64_t)fa.cw * fa.ch, 256)), dim3(256), 0, st, fa);
        return;
    }
    // small crops: 4 x as many (single-wave) workgroups; same sums, pixel by pixel
    const bool big = (uint64_t)div_up(fa.cw, 16) * div_up(fa.ch, 16) >= 4ull * (uint64_t)c->n_cu;
    const bool tent = fa.filter == PBRT_FILTER_TENT;
    const dim3 g16(div_up(fa.cw, 16), div_up(fa.ch, 16)), g8(div_up(fa.cw, 8), div_up(fa.ch, 8));
    if (big && tent)
        hipLaunchKernelGGL((k_film_accum_tiled<16, PBRT_FILTER_TENT>), g16, dim3(16, 16), 0, st, fa);
    else if (big)
        hipLaunchKernelGGL((k_film_accum_tiled<16, PBRT_FILTER_GAUSSIAN>), g16, dim3(16, 16), 0, st, fa);
    else if (tent)
        hipLaunchKernelGGL((k_film_accum_tiled<8, PBRT_FILTER_TENT>), g8, dim3(8, 8), 0, st, fa);
    else
        hipLaunchKernelGGL((k_film_accum_tiled<8, PBRT_FILTER_GAUSSIAN>), g8, dim3(8, 8), 0, st, fa);
}

// The fuse plan learnt from the probe pass of a render: its statistics rows reduced and read back (one synchronisation, ~30 us); the
// reduction target is cleared again, the final reduction adds every row once more
static int probe_plan(pbrt_ctx *c, unsigned long long *segstats, uint32_t n_rows, uint32_t stat_rows, unsigned long long *dstats,
                      uint32_t max_depth, uint32_t *plan) {
    hipStream_t st = c->stream;
    unsigned long long hp[2 + MAX_DEPTH_STATS];
    hipLaunchKernelGGL(k_reduce_stats, dim3(stat_rows, REDUCE_SLICES), dim3(256), 0, st, segstats, n_rows, (size_t)n_rows, dstats);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hp, dstats, (size_t)stat_rows * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipMemsetAsync(dstats, 0, (2 + 2 * MAX_DEPTH_STATS) * 8, st));
    for (uint32_t d = stat_rows; d < 2 + MAX_DEPTH_STATS; ++d) hp[d] = 0;
    *plan = plan_from_survival(hp + 2, std::min<uint32_t>(max_depth, MAX_DEPTH_STATS));
    return PBRT_OK;
}

// What the stages of a radiance render share.  render_impl calls the stages in order; each fills its own group of members.
namespace {
struct Render {
    pbrt_scene *s;
    pbrt_ctx *c;
    const pbrt_camera *cam;
    const pbrt_film_desc *f;
    void *d_out;
    // render_check: the request (render_request.h: the rules, the launch structure, the rendered region, the row counts), the switches
    RenderRequest rq;
    Switches sw;
    // render_buffers: the shape of a full pass (n_own: its live counters, n_rows: its statistics rows) and the buffers of the call
    PassShape ps;
    uint32_t n_own = 0, n_rows = 0;
    WfBufs wfb{};
    WfPlan wfp;
    float *Lhome = nullptr, *acc = nullptr;
    uint32_t *segA = nullptr, *segB = nullptr;
    unsigned long long *dstats = nullptr, *segstats = nullptr;
    // render_plan: the fuse plan of the call (plan: of the passes after the probe pass, once that has run)
    FusePlan fp;
    // render_args: the arguments of every pass
    RadArgs base{};
    FilmArgs fa{};
    // the pass loop
    PassTimer timer{};
    uint32_t passes = 0, launches = 0;
    // render_finish: the reduced statistics rows and the guard words of the call, read back
    unsigned long long hstats[2 + 2 * MAX_DEPTH_STATS];
    uint32_t hguard[WF_GUARD_WORDS] = {0};
};
}  // namespace

// What the scene's accelerator decides for a request (render_request.h RenderLaunch)
static RenderLaunch render_launch(const pbrt_scene *s) {
    static_assert(WF_REGION == REGION_SEGS_BVH * SEG_BVH, "both BVH launch structures cut a pass into the same regions");
    const int k = s->accel_kernel;
    RenderLaunch l;
    l.brute = k == ACCEL_K_BRUTE || k == ACCEL_K_BRUTE_BIG;
    l.keep = k == ACCEL_K_BRUTE && s->ds.n_prims <= 32;
    l.region = rad_region_segs(k) * seg_threads(k);
    l.owners = rad_owners_per_region(k);
    l.rows_fused = k == ACCEL_K_BRUTE ? std::max(rad_rows_per_region(k), path_groups_per_region()) : rad_rows_per_region(k);  // (launch_path)
    l.rows_streams = WF_SHADE_THREADS / 64u;
    return l;
}

// Check: the context settled, the request made (the argument rules, the launch structure of the scene, the rendered region), the
// device, the switches.
static int render_check(Render &r) {
    pbrt_ctx *c = r.c;
    if (int rcs = ctx_settle(c)) return rcs;
    if (const char *why = render_request(&r.rq, r.cam, r.f, r.d_out != nullptr, render_launch(r.s))) return RULE_TEXT(c, why);
    HIPCHK(c, hipSetDevice(c->device));
    r.sw = read_switches();
    return PBRT_OK;
}

// Pass sizing and buffers: the paths in flight per pass, the buffers whose size follows it, the counters, the film accumulator and
// the statistics rows; the launch shape of the streams.
static int render_buffers(Render &r) {
    pbrt_scene *s = r.s;
    pbrt_ctx *c = r.c;
    const pbrt_film_desc *f = r.f;
    const RenderRequest &rq = r.rq;
    const bool wavefront = rq.wavefront;
    // default paths in flight per pass, measured on cbox 512^2 x 256 (one box): 2 / 4 / 8 / 16 / 32 / 64 Mi -> 9.55 / 8.56 / 8.14 / 7.92 /
    // 8.13 / 8.20 ms (fewer launch tails against cache residency of the ping-pong state)
    // round 2, fused first launch: 2 / 4 / 8 / 16 / 32 / 64 Mi -> 9.09 / 8.07 / 7.65 / 7.37 / 7.31 / 7.39 ms; BVH scenes keep 16 Mi
    // round 2, chains of up to six bounces per launch (one launch per pass on the Cornell box): 2 / 4 / 8 / 16 / 32 / 64 Mi -> 7.85 / 7.01 /
    // 6.72 / 6.56 / 6.49 / 6.43 ms
    // round 3, BVH scenes as trace / shade streams (twelve launches per pass: their tails and the thinly filled late bounces weigh
    // less in larger passes): ring 1024^2 x 64: 1 / 2 / 4 / 8 / 16 / 32 / 64 Mi -> 50.8 / 37.6 / 25.5 / 22.2 / 19.6 / 18.0 / 17.3 ms;
    // 64 Mi paths = 23 GB of workspace (356 B per path in flight then, 340 B since round 4); the fused BVH kernels (PBRT_FILM_NO_HIT_POOL) keep 16 Mi
    // and beyond: 1024^2 x 512: 64 / 128 / 256 Mi -> 144 / 134 / 115 ms.  Default for BVH scenes: the largest power of two whose
    // workspace (WF_BYTES_PER_PATH = 340 B per path in flight, allocated as asked) fits two thirds of the free device memory and
    // the context's workspace limit, 1 .. 512 Mi (round 4, 1024^2 x 512: 128 / 256 / 512 Mi -> 105.9 / 99.5 / 94.6 ms; 512 Mi paths =
    // 183 GB of the 288 GB of an MI355X -- a renderer that owns the device takes it; one that shares it sets a limit, see
    // pbrt_ctx_set_workspace_limit, and pbrt_ctx_trim hands the memory back).  A failed allocation halves the pass (size_pass).
    // Brute-force scenes under a workspace limit: 16 B of radiance record per path, and the ping-pong state (2 x 60 B) if the
    // launch plan turns out to need it.
    // (pbrt_ctx::call_seq was bumped by the entry point, before its first workspace request.)
    const uint64_t pass_paths = f->pass_paths ? f->pass_paths
                                              : default_pass_paths(c, wavefront, rq.brute ? (64u << 20) : (16u << 20), 16 + 2 * N_STATE * 4);
    auto alloc_pass = [&](const PassShape &ps) -> int {
        r.Lhome = (float *)c->buf("Lhome", (size_t)ps.cap * 16);  // float4 (r, g, b, 0) per home
        return r.Lhome && (!wavefront || wf_alloc(c, ps.cap, ps.nseg, &r.wfb)) ? PBRT_OK : PBRT_E_NOMEM;
    };
    int rc = size_pass(c, pass_paths, f->pass_paths != 0, f->spp, rq.npix_r, rq.launch.region, true, wavefront, N_STATE, alloc_pass, &r.ps);
    if (rc) return rc;
    if (wavefront) {
        r.wfp = wf_plan(s, r.sw);
        if ((rc = wf_set_attr(s, r.wfp)) != 0) return rc;
    }
    // live counters and statistics rows: one per region, or one per wave of it (BVH kernels: wave-private compaction)
    r.n_own = r.ps.nseg * rq.launch.owners;
    r.n_rows = r.ps.nseg * rq.rows_per_region();
    r.segA = (uint32_t *)c->buf("segA", (size_t)r.n_own * 4);
    r.segB = (uint32_t *)c->buf("segB", (size_t)r.n_own * 4);
    r.acc = (float *)c->buf("film_acc", rq.film_px * 16);
    r.dstats = (unsigned long long *)c->buf("stats", (2 + 2 * MAX_DEPTH_STATS) * 8);
    r.segstats = (unsigned long long *)c->buf("segstats", (size_t)(2 + 2 * MAX_DEPTH_STATS) * r.n_rows * 8);
    if (!r.segstats) return PBRT_E_NOMEM;
    return r.Lhome && r.segA && r.segB && r.acc && r.dstats ? PBRT_OK : PBRT_E_NOMEM;
}

// What the call clears -- the film accumulator, the reduction target, the statistics rows in use (cleared and reduced per call:
// kept to what the call touches) -- and the start of its clock.
static int render_clear(Render &r) {
    pbrt_ctx *c = r.c;
    const RenderRequest &rq = r.rq;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemsetAsync(r.acc, 0, rq.film_px * 16, st));
    HIPCHK(c, hipMemsetAsync(r.dstats, 0, (2 + 2 * MAX_DEPTH_STATS) * 8, st));
    HIPCHK(c, hipMemsetAsync(r.segstats, 0, (size_t)rq.stat_rows * r.n_rows * 8, st));
    if (rq.hit_rows) HIPCHK(c, hipMemsetAsync(r.segstats + (size_t)HIT_ROW0 * r.n_rows, 0, (size_t)rq.hit_rows * r.n_rows * 8, st));
    HIPCHK(c, hipEventRecord(c->ev0, st));
    r.timer = PassTimer{c};
    return PBRT_OK;
}

// The fuse plan of this call and whether a probe pass is to learn it (render_request.h fuse_plan)
static void render_plan(Render &r, bool may_probe = true) {
    r.fp = fuse_plan(r.rq, r.s->plan_hint_valid, r.s->plan_hint, r.ps.per_pass, may_probe);
}

// Argument blocks: what every pass hands its bounce kernels (key_mode 0: home -> (pixel of the rendered region, sample s_first +
// home / npix_r)) and the film gather.
static int render_args(Render &r) {
    pbrt_scene *s = r.s;
    const pbrt_film_desc *f = r.f;
    const uint32_t rw = r.rq.rw, cap = r.ps.cap;
    RadArgs &base = r.base;
    base.sc = s->ds;
    if ((f->flags & PBRT_FILM_NO_OCCLUDER_PRUNING) && base.sc.occ_prims) {  // diagnostic: shadow segments walk every primitive
        base.sc.occ_prims = base.sc.prims;
        base.sc.n_occ = base.sc.n_prims;
        base.sc.occ_runs = base.sc.prim_runs;
        base.sc.n_occ_runs = base.sc.n_prim_runs;
        base.sc.occ_ord = base.sc.prim_ord;
    }
    if (f->flags & PBRT_FILM_NO_ORDERED_WALK) base.sc.prim_ord = base.sc.occ_ord = 0u;  // diagnostic: the table-walk instances (launch_bounce)
    base.cam = *r.cam;
    base.Lhome = r.Lhome;
    base.stats = r.segstats;
    base.stat_stride = r.n_rows;
    base.cap = cap;
    base.state_cap = cap;
    base.max_depth = f->max_depth;
    base.rr_depth = f->rr_depth;
    base.seed = f->seed;
    base.key_mode = 0;
    const FilmKey &key = base.key = render_film_key(r.rq);  // (s_first: the pass loop's)
    const std::initializer_list<uint32_t> probes = {0u, 1u, rw - 1, rw, rw + 1, key.npix_r - 1, key.npix_r, key.npix_r + 1, cap - 1, cap, 0xffffffffu};
    NEED(r.c, fastdiv_exact(key.div_npix, key.npix_r, probes) && fastdiv_exact(key.div_rw, rw, probes));
    base.lds_bytes = s->lds_bytes;
    base.tile_keep = nullptr;
    return PBRT_OK;
}
// ... and the film gather
static void render_film(Render &r) {
    const pbrt_film_desc *f = r.f;
    FilmArgs &fa = r.fa;
    fa.Lhome = r.Lhome;
    fa.acc = r.acc;
    fa.cap = r.ps.cap;
    fa.cx0 = f->crop_x;
    fa.cy0 = f->crop_y;
    fa.cw = f->crop_w;
    fa.ch = f->crop_h;
    fa.key = r.base.key;
    fa.rh = r.rq.rh;
    fa.filter = f->filter;
    fa.seed = f->seed;
}

// The keep words of the camera tiles (kernels_radiance.h k_tile_keep) for the requests that may carry them: built when the scene,
// the camera, the region or the buffer is not what the context's table was built for (camera and crop are the call's)
static int render_tile_keep(Render &r) {
    pbrt_ctx *c = r.c;
    c->tile_keep_last = false;
    if (!r.rq.tile_keep) return PBRT_OK;
    TileKeepArgs ta;
    ta.prims = r.s->ds.prims;
    ta.n_prims = r.s->ds.n_prims;
    ta.cam = *r.cam;
    ta.key = r.base.key;
    ta.n_blocks = ta.key.npix_r / 64;
    ta.keep = (uint32_t *)c->buf("tile_keep", (size_t)ta.n_blocks * 4);
    if (!ta.keep) return PBRT_E_NOMEM;
    const pbrt_ctx::TileKeepKey key{c->work.generation("tile_keep"), r.s->serial, *r.cam, r.rq.rx0, r.rq.ry0, r.rq.rw, r.rq.rh};
    if (!(key == c->tile_keep_key)) {
        hipLaunchKernelGGL(k_tile_keep, dim3(div_up(ta.n_blocks, 64)), dim3(64), 0, c->stream, ta);
        HIPCHK(c, hipGetLastError());
        ++c->tile_keep_builds;
        c->tile_keep_key = key;
    }
    r.base.tile_keep = ta.keep;
    c->tile_keep_last = true;
    c->tile_keep_words = ta.keep;
    return PBRT_OK;
}

// The bounce launches of the fused brute-force kernels over nseg_pass regions: the launches of the fuse plan, each walking chain_len
// bounces, between the state sets in / out and the counters sin / sout (n_own of them).  camera: depth 0 generates its rays from the
// film keys (else the rays are in `in` / sin).  At most `bound` bounces, whatever a.max_depth says.
// path_ok: a launch of camera paths that walks every bounce of the pass may be k_path's (launch_path; PBRT_FILM_NO_PATH_KERNEL says no).
static int brute_bounces(pbrt_scene *s, RadArgs a, uint32_t plan, uint32_t nseg_pass, bool camera, uint32_t bound, float *in, float *out,
                         uint32_t *sin, uint32_t *sout, uint32_t n_own, uint32_t *launches, bool path_ok = false) {
    pbrt_ctx *c = s->ctx;
    int rc;
    for (uint32_t depth = 0; depth < a.max_depth && depth < bound;) {
        // bounces this launch walks: 2 at the depths of the fuse plan (the last bounce of a path only looks for emitters, so it
        // is never worth a launch slot of its own either)
        const uint32_t nb = chain_len(plan, depth, a.max_depth);
        a.depth = depth;
        a.nb = nb;
        a.in = in;
        a.out = out;
        a.seg_in = sin;
        a.seg_out = sout;
        const PathKern whole = path_ok && camera && depth == 0 && nb >= a.max_depth ? path_kernel(s, a.sc.prim_ord != 0u) : nullptr;
        if ((rc = whole ? launch_path(s, whole, a, nseg_pass) : launch_bounce(s, a, nseg_pass, camera && depth == 0, nb)) != 0) return rc;
        HIPCHK(c, hipGetLastError());
        ++*launches;
        std::swap(in, out);
        std::swap(sin, sout);
        const uint32_t depth_before = depth;
        depth += nb;
        bool dead;
        if ((rc = poll_live(c, a.max_depth, depth_before, depth, sin, n_own, &dead)) != 0) return rc;
        if (dead) break;
    }
    return PBRT_OK;
}

// The bounces of one pass of a brute-force scene.
// The ping-pong path state (2 x 60 B per slot, 8 GB at 64 Mi paths) is only touched by a pass that needs more than one bounce
// launch; with the plan that walks every bounce in one launch (the Cornell box) it is never written, so it is allocated per pass, for
// the paths of THAT pass, when its plan says so.
// A pass walks at most PASS_MAX_BOUNCES bounces whatever max_depth says (Mitsuba's -1 arrives as 0xffffffff) and drops the paths
// that are still alive then.  An unbounded render relies on it: poll_live sums the n_own counters of a FULL pass, and a shorter
// pass (the probe pass, a short last pass) leaves those of the regions it did not launch as an earlier call wrote them -- the
// survivors of a bounded render, for one -- so the sum may never reach 0 although every path of the pass has ended.  The launches
// up to the bound then find their regions empty.
constexpr uint32_t PASS_MAX_BOUNCES = 256;
static int brute_pass(Render &r, RadArgs a, uint32_t nseg_pass) {
    pbrt_ctx *c = r.c;
    const uint32_t region = r.rq.launch.region;
    const bool one_launch = chain_len(r.fp.plan, 0, a.max_depth) >= a.max_depth;
    const size_t need = one_launch ? (size_t)region : (size_t)nseg_pass * region;
    float *in = (float *)c->buf("stateA", need * N_STATE * 4), *out = (float *)c->buf("stateB", need * N_STATE * 4);
    if (!in || !out) return PBRT_E_NOMEM;
    a.state_cap = (uint32_t)need;
    if (int rc = r.timer.begin()) return rc;
    return brute_bounces(r.s, a, r.fp.plan, nseg_pass, true, PASS_MAX_BOUNCES, in, out, r.segA, r.segB, r.n_own, &r.launches,
                         !(r.f->flags & PBRT_FILM_NO_PATH_KERNEL));
}

// Pass loop: the samples in the passes of the schedule (render_request.h PassSchedule: the probe pass first, if the plan is to be
// learnt), each through the bounces of its launch structure and into the film accumulator.
static int render_passes(Render &r) {
    pbrt_ctx *c = r.c;
    const pbrt_film_desc *f = r.f;
    int rc;
    for (PassSchedule p{f->spp, r.ps.per_pass, r.fp.probe}; p.next(); ++r.passes) {
        RadArgs a = r.base;
        a.n_paths = (uint32_t)(r.rq.npix_r * p.sc);
        a.key.s_first = f->sample_offset + p.s0;
        const uint32_t nseg_pass = div_up(a.n_paths, r.rq.launch.region);
        if (r.rq.wavefront) {
            if ((rc = r.timer.begin()) != 0) return rc;
            rc = wf_bounces(r.s, wf_args(a), r.wfb, r.wfp, nseg_pass, true, &r.launches);
        } else {
            rc = brute_pass(r, a, nseg_pass);
        }
        if (rc) return rc;
        if ((rc = r.timer.end()) != 0) return rc;
        r.fa.key.s_first = a.key.s_first;
        r.fa.s_count = p.sc;
        film_accum(c, r.fa);
        HIPCHK(c, hipGetLastError());
        // learn the plan from the probe pass
        if (p.probing() && (rc = probe_plan(c, r.segstats, r.n_rows, r.rq.stat_rows, r.dstats, f->max_depth, &r.fp.plan)) != 0) return rc;
    }
    return PBRT_OK;
}

// Finish: the film resolved into d_out, the statistics rows reduced and read back with the guard words.
static int render_finish(Render &r) {
    pbrt_ctx *c = r.c;
    const RenderRequest &rq = r.rq;
    const uint32_t n_rows = r.n_rows;
    hipStream_t st = c->stream;
    int rc;
    hipLaunchKernelGGL(k_film_resolve, dim3(div_up(rq.film_px, 256)), dim3(256), 0, st, r.acc, (float *)r.d_out, (uint32_t)rq.film_px,
                       (uint32_t)(rq.out_floats == 4 ? 1 : 0));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, st));
    hipLaunchKernelGGL(k_reduce_stats, dim3(rq.stat_rows, REDUCE_SLICES), dim3(256), 0, st, r.segstats, n_rows, (size_t)n_rows, r.dstats);
    if (rq.hit_rows)
        hipLaunchKernelGGL(k_reduce_stats, dim3(rq.hit_rows, REDUCE_SLICES), dim3(256), 0, st, r.segstats + (size_t)HIT_ROW0 * n_rows, n_rows,
                           (size_t)n_rows, r.dstats + HIT_ROW0);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(r.hstats, r.dstats, sizeof r.hstats, hipMemcpyDeviceToHost, st));
    if (rq.wavefront && (rc = wf_guard_fetch(c, r.hguard)) != 0) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    return rq.wavefront ? wf_check_guard(c, r.hguard) : PBRT_OK;
}

// pbrt_stats filled (the plan that ran and where it came from, the byte model), and the plan this scene's next render starts from.
static int render_stats(Render &r) {
    pbrt_ctx *c = r.c;
    const unsigned long long *hstats = r.hstats;
    if (int rc = call_stats(c, hstats, r.rq.npix_r * r.f->spp, r.launches, r.passes, true, r.timer.n_ev)) return rc;
    pbrt_stats &S = c->stats;
    S.fuse_plan = r.fp.plan;
    S.plan_source = r.fp.source;
    S.pass_paths = (uint64_t)r.rq.npix_r * r.ps.per_pass;
    if (r.rq.brute && hstats[2] > 0) {  // remember what this scene's paths do for the next render of it
        r.s->plan_hint = plan_from_survival(hstats + 2, (uint32_t)std::min<uint64_t>(r.f->max_depth, MAX_DEPTH_STATS));
        r.s->plan_hint_valid = true;
    }
    const ModelBytes m = render_model_bytes(r.rq, hstats, S.samples, r.passes, r.fp.plan);
    S.model_bytes = m.total;
    S.bounce_model_bytes = m.bounce;
    if (r.rq.wavefront) S.trace_model_bytes = m.trace;
    return PBRT_OK;
}

#ifdef PBRT_DIAG
#include "diag_driver.h"  // diag_selected, diag_render: the launch structures only the diagnostic build carries
#endif

static int render_impl(pbrt_scene *s, const pbrt_camera *cam, const pbrt_film_desc *f, void *d_out) {
    Render r{s, s->ctx, cam, f, d_out};
    int rc;
    if ((rc = render_check(r)) != 0) return rc;
    // launch structures that lost their A/B live in the diagnostic build only (make -C csrc diag -> libpbrt_hip_diag.so)
#ifdef PBRT_DIAG
    if (diag_selected(r)) return diag_render(r);
#else
    if ((f->flags & (PBRT_FILM_REGEN | PBRT_FILM_WALK_SET)) || (!r.rq.brute && (f->flags & PBRT_FILM_NO_HIT_POOL)))
        return r.c->fail(PBRT_E_UNSUPPORTED, "PBRT_FILM_REGEN / PBRT_FILM_WALK_FROM / PBRT_FILM_NO_HIT_POOL select diagnostic launch "
                                             "structures: build libpbrt_hip_diag.so (make -C csrc diag)");
#endif
    if ((rc = render_buffers(r)) != 0) return rc;
    if ((rc = render_clear(r)) != 0) return rc;
    render_plan(r);
    if ((rc = render_args(r)) != 0) return rc;
    if ((rc = render_tile_keep(r)) != 0) return rc;
    render_film(r);
    if ((rc = render_passes(r)) != 0) return rc;
    if ((rc = render_finish(r)) != 0) return rc;
    return render_stats(r);
}

#ifdef PBRT_BVH_PROBE  // diagnostic builds only (tools/bvh_probe.py); not part of the ABI
extern "C" int pbrt_debug_bvh_probe(unsigned long long *out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bvh_probe), 64) != hipSuccess) return PBRT_E_DEVICE;
    if (reset) {
        unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_bvh_probe), z, 64) != hipSuccess) return PBRT_E_DEVICE;
    }
    return PBRT_OK;
}
#endif

// ---- pbrt_integrator_sample: radiance along the caller's rays, on the pieces of a render ------------------------------------------
// One pass of n paths (no halving) whose first bounce reads the rays from the state instead of generating them; key_mode 1: the key
// of ray i is (index_offset + i, sample_index).
namespace {
struct SampleCall {
    pbrt_scene *s;
    pbrt_ctx *c;
    uint32_t n;
    const float *o, *d, *tmax;
    uint32_t index_offset, sample_index, seed, max_depth, rr_depth;
    float *rgb;
    // sample_check
    Switches sw;
    RenderLaunch launch;
    bool streams = false;  // trace / shade streams
    // sample_buffers: the pass, its counters and rows, what differs between the two launch structures (path state and live counters),
    // the radiance records, the statistics rows (k_shade: and its hit rows), the caller's rays on the device
    PassShape ps;
    uint32_t n_own = 0, n_rows = 0;
    WfBufs wfb{};
    WfPlan wfp;
    float *stA = nullptr, *stB = nullptr, *Lhome = nullptr, *dO = nullptr, *dD = nullptr, *dT = nullptr;
    uint32_t *segA = nullptr, *segB = nullptr;
    unsigned long long *dstats = nullptr, *rows = nullptr;
    size_t rows_bytes = 0;
    RadArgs a{};
    uint32_t hguard[WF_GUARD_WORDS] = {0};
};
}  // namespace

static int sample_check(SampleCall &q) {
    pbrt_ctx *c = q.c;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rcs = ctx_settle(c)) return rcs;
    ++c->call_seq;
    q.sw = read_switches();
    q.launch = render_launch(q.s);
    q.streams = !q.launch.brute;
    return one_pass(c, q.n, 1, q.n, q.launch.region, false, q.streams, N_STATE, &q.ps);
}

static int sample_buffers(SampleCall &q) {
    pbrt_scene *s = q.s;
    pbrt_ctx *c = q.c;
    const uint32_t cap = q.ps.cap, nseg = q.ps.nseg;
    q.n_own = nseg * q.launch.owners;
    if (q.streams) {
        if (!wf_alloc(c, cap, nseg, &q.wfb)) return PBRT_E_NOMEM;
        q.wfp = wf_plan(s, q.sw);
        if (int rc = wf_set_attr(s, q.wfp)) return rc;
    } else {
        q.stA = (float *)c->buf("stateA", (size_t)cap * N_STATE * 4);
        q.stB = (float *)c->buf("stateB", (size_t)cap * N_STATE * 4);
        q.segA = (uint32_t *)c->buf("segA", (size_t)q.n_own * 4);
        q.segB = (uint32_t *)c->buf("segB", (size_t)q.n_own * 4);
        q.dstats = (unsigned long long *)c->buf("stats", (2 + MAX_DEPTH_STATS) * 8);
        if (!q.stA || !q.stB || !q.segA || !q.segB || !q.dstats) return PBRT_E_NOMEM;
    }
    q.Lhome = (float *)c->buf("Lhome", (size_t)cap * 16);  // float4 (r, g, b, 0) per home
    q.n_rows = nseg * (q.streams ? q.launch.rows_streams : q.launch.rows_fused);
    q.rows_bytes = (size_t)(2 + (q.streams ? 2 : 1) * MAX_DEPTH_STATS) * q.n_rows * 8;
    q.rows = (unsigned long long *)c->buf("segstats", q.rows_bytes);
    const size_t n = q.n;
    const auto io_at = stage_layout(stage_in(q.o, 3 * n), stage_in(q.d, 3 * n), stage_in(q.tmax, n));
    char *io = (char *)c->buf("leaf_io", io_at.total);
    if (!q.Lhome || !q.rows || !io) return PBRT_E_NOMEM;
    q.dO = (float *)(io + io_at.offset[0]);
    q.dD = (float *)(io + io_at.offset[1]);
    q.dT = (float *)(io + io_at.offset[2]);
    return PBRT_OK;
}

// the rays uploaded, and what the call clears
static int sample_upload(SampleCall &q) {
    pbrt_ctx *c = q.c;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(q.dO, q.o, (size_t)q.n * 12, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(q.dD, q.d, (size_t)q.n * 12, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(q.dT, q.tmax, (size_t)q.n * 4, hipMemcpyHostToDevice, st));
    if (q.dstats) HIPCHK(c, hipMemsetAsync(q.dstats, 0, (2 + MAX_DEPTH_STATS) * 8, st));
    HIPCHK(c, hipMemsetAsync(q.rows, 0, q.rows_bytes, st));
    HIPCHK(c, hipMemsetAsync(q.Lhome, 0, (size_t)q.ps.cap * 16, st));
    return PBRT_OK;
}

// the film key of key mode 1, which has no film: path_key does not read it, and the two divisions by 1 stand where a render's are
static FilmKey sample_key() {
    FilmKey k{};
    k.npix_r = k.rw = 1;
    k.div_npix = k.div_rw = make_fastdiv(1);
    return k;
}
// key_mode 1: key = (index_offset + home, sample_index) for the caller's n rays
static void sample_args(SampleCall &q) {
    RadArgs &a = q.a;
    a.sc = q.s->ds;
    a.Lhome = q.Lhome;
    a.stats = q.rows;
    a.stat_stride = q.n_rows;
    a.cap = q.ps.cap;
    a.state_cap = q.ps.cap;
    a.n_paths = q.n;
    a.max_depth = q.max_depth;
    a.rr_depth = q.rr_depth;
    a.seed = q.seed;
    a.key_mode = 1;
    a.key = sample_key();
    a.index_offset = q.index_offset;
    a.sample_index = q.sample_index;
    a.lds_bytes = q.s->lds_bytes;
}

// the rays into the state of their launch structure, and its bounces: the streams', or the fused kernels' with one launch per bounce
// and as many bounces as the paths live (a single full pass: every counter poll_live sums is this call's)
static int sample_bounces(SampleCall &q) {
    pbrt_scene *s = q.s;
    const uint32_t n = q.n, cap = q.ps.cap, nseg = q.ps.nseg, n_own = q.n_own;
    hipStream_t st = q.c->stream;
    uint32_t launches = 0;
    if (q.streams) {
        hipLaunchKernelGGL(k_init_rays_wf, dim3(div_up(std::max(n, nseg), 256)), dim3(256), 0, st, q.wfb.stA, cap, q.wfb.segA, nseg, n, q.dO, q.dD, q.dT);
        if (int rc = wf_bounces(s, wf_args(q.a), q.wfb, q.wfp, nseg, false, &launches)) return rc;
        return wf_guard_fetch(q.c, q.hguard);
    }
    hipLaunchKernelGGL(k_init_rays, dim3(div_up(std::max(n, n_own), 256)), dim3(256), 0, st, q.stA, q.segA, n_own,
                       q.launch.region / q.launch.owners, n, q.dO, q.dD, q.dT);
    return brute_bounces(s, q.a, 0u, nseg, false, q.max_depth, q.stA, q.stB, q.segA, q.segB, n_own, &launches);
}

static int sample_read(SampleCall &q) {
    pbrt_ctx *c = q.c;
    const uint32_t n = q.n;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (q.streams)
        if (int rc = wf_check_guard(c, q.hguard)) return rc;
    std::vector<float> rec((size_t)n * 4);
    HIPCHK(c, hipMemcpy(rec.data(), q.Lhome, (size_t)n * 16, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) q.rgb[(size_t)k * n + i] = rec[(size_t)i * 4 + k];
    return PBRT_OK;
}

extern "C" {

int pbrt_render_radiance_dev(pbrt_scene *s, const pbrt_camera *cam, const pbrt_film_desc *f, void *d_out) {
    if (!s) return PBRT_E_INVALID;
    ++s->ctx->call_seq;
    return render_impl(s, cam, f, d_out);
}

// (the request is made here as well, before anything is asked of the workspace: film_out takes its size from it)
int pbrt_render_radiance(pbrt_scene *s, const pbrt_camera *cam, const pbrt_film_desc *f, float *out) {
    if (!s) return PBRT_E_INVALID;
    pbrt_ctx *c = s->ctx;
    NEED(c, cam && f && out);
    RenderRequest rq;
    if (const char *why = render_request(&rq, cam, f, true, render_launch(s))) return RULE_TEXT(c, why);
    HIPCHK(c, hipSetDevice(c->device));
    ++c->call_seq;
    const size_t n = (size_t)rq.film_px * rq.out_floats;
    void *d = c->buf("film_out", n * 4);
    if (!d) return PBRT_E_NOMEM;
    int rc = render_impl(s, cam, f, d);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(out, d, n * 4, hipMemcpyDeviceToHost));
    return PBRT_OK;
}

int pbrt_integrator_sample(pbrt_scene *s, uint32_t n, const float *o, const float *d, const float *tmax,
                           uint32_t index_offset, uint32_t sample_index, uint32_t seed, uint32_t max_depth,
                           uint32_t rr_depth, float *rgb) {
    if (!s) return PBRT_E_INVALID;
    NEED(s->ctx, o && d && tmax && rgb && max_depth > 0);
    if (n == 0) return PBRT_OK;
    SampleCall q{s, s->ctx, n, o, d, tmax, index_offset, sample_index, seed, max_depth, rr_depth, rgb};
    int rc;
    if ((rc = sample_check(q)) != 0) return rc;
    if ((rc = sample_buffers(q)) != 0) return rc;
    if ((rc = sample_upload(q)) != 0) return rc;
    sample_args(q);
    if ((rc = sample_bounces(q)) != 0) return rc;
    return sample_read(q);
}

// ------------------------------------------------------------------------------------------------
// ultrasound mode driver
// ------------------------------------------------------------------------------------------------
// The curved array (PBRT_US_ARRAY_CONVEX, DESIGN D18).  The geometry is CustomEmitter's (CustomEmmitter.py:41-47), evaluated with the
// float statements of kernels_us.h us_emitter_ray, so that the position an emitter ray starts from and the position the receive
// connection aims at are the same floats (sin / cos: kernels_us.h emit_sincos itself, compiled for the host -- the polynomial of
// device_math.h sincos_pi4 up to 45 degrees; beyond, the host's sinf / cosf where the kernel calls the device library's, which agree
// to a few ulp).  Its rules: us_request.h us_array_rules.
// element e of the array: (x, z, nx, nz) in the sensor's frame
static void us_array_element(const pbrt_us_params *p, uint32_t e, float *out) {
    if (!us_convex(p)) {
        out[0] = us_elem_x(p, e);
        out[1] = 0.0f;
        out[2] = 0.0f;
        out[3] = 1.0f;
        return;
    }
    const float N = (float)p->n_elements, idx = (float)e;
    const float span = p->emitter.opening_angle * (K_PI / 180.0f);                            // CustomEmmitter.py:42
    const float lo = -span / 2.0f, hi = span / 2.0f;
    const float th = N > 1.0f ? host_fma(idx, (hi - lo) / (N - 1.0f), lo) : lo;               // :43
    float sth, cth;
    emit_sincos(th, &sth, &cth);  // (kernels_us.h: the one text host and kernels share)
    out[0] = p->emitter.radius * sth;                                                         // :44-46
    out[1] = p->emitter.radius * cth;
    out[2] = sth;                                                                             // :47
    out[3] = cth;
}

int pbrt_us_array_elements(const pbrt_us_params *p, float *elem) {
    if (!p || !elem || p->n_elements == 0) return PBRT_E_INVALID;
    if (us_convex(p) && us_array_rules(p)) return PBRT_E_INVALID;
    for (uint32_t e = 0; e < p->n_elements; ++e) us_array_element(p, e, elem + 4 * (size_t)e);
    return PBRT_OK;
}

int pbrt_us_tx_delays(const pbrt_us_params *p, float *tx) {
    if (!p || !tx || p->n_angles > PBRT_US_MAX_ANGLES || p->n_angles == 0 || p->n_elements == 0) return PBRT_E_INVALID;
    if (us_convex(p)) {  // the plane wave along (sin a, 0, cos a), referenced to the apex (0, 0, R): (x_e sin a + (z_e - R) cos a) / c
        if (us_array_rules(p)) return PBRT_E_INVALID;
        for (uint32_t a = 0; a < p->n_angles; ++a) {
            const double ar = (double)p->angles_deg[a] * (M_PI / 180.0);
            for (uint32_t e = 0; e < p->n_elements; ++e) {
                float el[4];
                us_array_element(p, e, el);
                tx[a * p->n_elements + e] = (float)(((double)el[0] * std::sin(ar) + ((double)el[1] - (double)p->emitter.radius) * std::cos(ar)) /
                                                    (double)p->sound_speed);
            }
        }
        return PBRT_OK;
    }
    for (uint32_t a = 0; a < p->n_angles; ++a) {
        double ar = (double)p->angles_deg[a] * (M_PI / 180.0);  // np.deg2rad, CustomIntegrator.py:247
        for (uint32_t e = 0; e < p->n_elements; ++e) {
            // :254,257 tx = f32(elem_x * sin(a) / c)
            const float ex = us_elem_x(p, e);
            tx[a * p->n_elements + e] = (float)(((double)ex * std::sin(ar)) / (double)p->sound_speed);
        }
    }
    return PBRT_OK;
}

}  // extern "C"

// which instance of k_us_bounce: the switches of the library's default (with / without the carrier) are compiled in, any other set
// -- and PBRT_US_GENERIC_KERNEL=1 -- takes the instance that reads them at run time (kernels_us.h)
static uint32_t us_kernel_quirks(const UsArgs &a, bool generic) {
    if (generic) return US_Q_RUNTIME;
    const uint32_t host_only = PBRT_USQ_NO_FIRST_TABLES | PBRT_USQ_NO_FUSED_BOUNCES;  // decided on the host: tables null, a.fuse 0
    const uint32_t q = a.p.quirks & ~host_only;
    return (q == PBRT_USQ_REFERENCE || q == (PBRT_USQ_REFERENCE | PBRT_USQ_NO_CARRIER)) ? q : US_Q_RUNTIME;
}
static int launch_us(pbrt_scene *s, const UsArgs &a, uint32_t nseg, bool first, bool generic, bool convex) {
    const bool emit = a.p.primary == PBRT_US_PRIMARY_EMITTER;  // primary rays from CustomEmitter.sample_ray, echoes times the ray's weight
    const int tab = (a.first_hit && a.first_rx) ? 1 : (!a.first_hit && !a.first_rx) ? 0 : -1;
    UsKern k = us_bounce_kernel(s, first, emit, us_kernel_quirks(a, generic), tab, convex);
#ifdef PBRT_DIAG
    if (!k && !emit) k = diag_us_bvh_kernel(s, first, convex);
#endif
    if (!k && emit)
        return s->ctx->fail(PBRT_E_UNSUPPORTED, "launch_us: emitter primary rays on BVH scenes run as streams (us_wf_pass)");
    if (!k) return s->ctx->fail(PBRT_E_UNSUPPORTED, "launch_us: no fused ultrasound bounce for accelerator %d in this build", s->accel_kernel);
    const bool lds = s->accel_kernel == ACCEL_K_BVH_LDS;
    hipLaunchKernelGGL(k, dim3(nseg), dim3(seg_threads(s->accel_kernel)), lds ? s->lds_bytes : 0u, s->ctx->stream, a);
    return PBRT_OK;
}
// The kernels that meet one ray with the scene and nothing else (first-bounce tables, leaf operators): the brute-force loop over
// the full tables, or the tree in global memory
static bool brute_scene(const pbrt_scene *s) { return s->accel_kernel == ACCEL_K_BRUTE || s->accel_kernel == ACCEL_K_BRUTE_BIG; }
static UsFirstKern us_first_kernel(const pbrt_scene *s, bool convex) {
    return with_flags([](auto B, auto X) -> UsFirstKern { return &k_us_first<B() ? ACCEL_K_BRUTE_BIG : ACCEL_K_BVH_GLOBAL, X()>; },
                      brute_scene(s), convex);
}
static RayIntersectKern ray_intersect_kernel(const pbrt_scene *s) {
    return brute_scene(s) ? &k_ray_intersect<ACCEL_K_BRUTE_BIG> : &k_ray_intersect<ACCEL_K_BVH_GLOBAL>;
}
static RayTestKern ray_test_kernel(const pbrt_scene *s) {
    return brute_scene(s) ? &k_ray_test<ACCEL_K_BRUTE_BIG> : &k_ray_test<ACCEL_K_BVH_GLOBAL>;
}
// k_us_shade: first bounce from the tables, scene with cylinders, curved array
static UsWfKern us_shade_kernel(const pbrt_scene *s, bool tab, bool convex) {
    return with_flags([](auto T, auto C, auto X) -> UsWfKern { return &k_us_shade<T(), C(), X()>; }, tab, s->cylinders, convex);
}

// BVH scenes: the bounces of one ultrasound pass as k_trace / k_us_shade streams (kernels_us_wavefront.h).  a: the pass's UsArgs
// (cap, n_paths, ppr_pass, path_first, tables set).  One launch at depth 0 with the first-bounce tables (else k_us_init_wf +
// k_trace + k_us_shade), two per later bounce, and a flush for the occlusion rays of the last one.
static int us_wf_pass(pbrt_scene *s, UsArgs a, const WfBufs &b, const WfPlan &p, uint32_t nreg, bool convex, uint32_t *launches) {
    pbrt_ctx *c = s->ctx;
    hipStream_t st = c->stream;
    WfArgs t{};
    t.sc = s->ds;
    t.cap = a.cap;
    t.n_paths = a.n_paths;
    t.key_mode = 0;
    t.vis_q = US_WF_VIS_Q;
    if (!wf_tree_args(s, p, &t)) return PBRT_E_NOMEM;
    UsWfArgs w{};
    w.guard = t.guard;
    WfPing pp(b);
    auto trace = [&](uint32_t depth, bool have_shadows) {
        t.depth = depth;
        pp.bind(t, b, have_shadows, 0, nreg);
        wf_launch_trace(s, t, p, wf_trace_grid(nreg, depth >= 2 ? p.grid_deep : p.grid_mult, (uint32_t)c->n_cu, WF_KMAX), false, st);
        ++*launches;
    };
    auto shade = [&](uint32_t depth, bool tab, bool have_shadows) {
        a.depth = depth;
        w.u = a;
        pp.bind(w, b, have_shadows, 0, nreg);
        hipLaunchKernelGGL(us_shade_kernel(s, tab, convex), dim3(nreg), dim3(WF_SHADE_THREADS), 0, st, w);
        ++*launches;
    };
    const bool tab = a.first_hit != nullptr && a.first_rx != nullptr;
    if (tab) {
        shade(0, true, false);
    } else {
        hipLaunchKernelGGL(convex ? k_us_init_wf<true> : k_us_init_wf<false>, dim3(div_up(std::max(a.n_paths, nreg), 256)), dim3(256), 0, st, a, pp.in,
                           pp.sin, nreg);
        trace(0, false);
        shade(0, false, false);
    }
    pp.flip();
    HIPCHK(c, hipGetLastError());
    for (uint32_t depth = 1; depth < a.p.max_depth; ++depth) {
        trace(depth, true);
        shade(depth, false, true);
        pp.flip();
        HIPCHK(c, hipGetLastError());
    }
    // the occlusion rays of the last bounce (every path has ended: records of ended paths only), and their echoes
    trace(a.p.max_depth, true);
    shade(a.p.max_depth, false, true);
    HIPCHK(c, hipGetLastError());
    return PBRT_OK;
}

// What the stages of an acquisition share.  us_impl calls the stages in order; each fills its own group of members.
namespace {
struct Acquire {
    pbrt_scene *s;
    pbrt_ctx *c;
    const pbrt_us_params *p;
    uint32_t seed, ppr, path_offset, norm_paths;
    float *d_channel, *tx_host;
    bool wait;
    // us_check: the request (us_request.h: the rules, the derived facts, the host's constants), the switches, the launch structure
    UsRequest rq;
    bool timed = true;  // (event pairs recorded into a graph cannot be read back)
    Switches sw;
    bool streams = false;  // k_trace / k_us_shade streams (us_wf_pass), not the fused k_us_bounce
    // us_buffers: the shape of a full pass (n_own: its live counters / statistics rows) and the buffers of the call
    uint32_t region = 0, n_own = 0;
    PassShape ps;
    WfBufs wfb{};
    WfPlan wfp;
    float *stA = nullptr, *stB = nullptr;
    uint32_t *segA = nullptr, *segB = nullptr;
    unsigned long long *segstats = nullptr;
    size_t segstats_bytes = 0;
    float *tabs = nullptr;  // transmit delays [n_rays], primary directions [3 n_angles], elements [n_ex]; filled by us_tables
    // us_args: the arguments every pass shares (us_passes sets those of a pass, us_fused_pass those of a launch)
    UsArgs a{};
    // us_passes
    PassTimer timer{};
    uint32_t passes = 0, launches = 0;
};
// the buffers whose size follows the pass (size_pass: again with half the paths after a failed allocation)
struct UsAllocPass {
    Acquire &q;
    int operator()(const PassShape &ps) const {
        pbrt_ctx *c = q.c;
        if (q.streams) return wf_alloc(c, ps.cap, ps.nseg, &q.wfb) ? PBRT_OK : PBRT_E_NOMEM;
        q.stA = (float *)c->buf("stateA", (size_t)ps.cap * N_STATE * 4);
        q.stB = q.stA ? (float *)c->buf("stateB", (size_t)ps.cap * N_STATE * 4) : nullptr;
        return q.stA && q.stB ? PBRT_OK : PBRT_E_NOMEM;
    }
};
}  // namespace

// Check: what a recording admits, the argument rules and what follows from the block (us_request.h), the switches, the launch structure.
static int us_check(Acquire &q) {
    pbrt_ctx *c = q.c;
    if (c->recording) {  // recorded, not run: the queueing form only, one acquisition per recording
        if (q.wait || c->pend.active) return c->fail(PBRT_E_INVALID, "recording: one pbrt_us_acquire_queue_dev per recording, and no call that waits");
    } else if (int rcs = ctx_settle(c)) {
        return rcs;
    }
    q.timed = !c->recording;
    if (const char *why = us_request(&q.rq, q.p, q.ppr, q.d_channel != nullptr))
        return q.rq.code == PBRT_E_INVALID ? c->fail(PBRT_E_INVALID, "invalid argument: %s", why) : c->fail(q.rq.code, "%s", why);
    HIPCHK(c, hipSetDevice(c->device));
    q.sw = read_switches();
    // BVH scenes (tessellated phantoms, meshes) run as k_trace / k_us_shade streams (us_wf_pass); the diagnostic build keeps the
    // fused bounce behind PBRT_US_FUSED_BVH=1 for the A/B
    q.streams = q.s->accel_kernel == ACCEL_K_BVH_GLOBAL || q.s->accel_kernel == ACCEL_K_BVH_LDS;
#ifdef PBRT_DIAG
    if (int rc = diag_us_fused_bvh(q.s, &q.streams)) return rc;
#endif
    return PBRT_OK;
}

// Pass sizing and buffers: the paths in flight per pass and the buffers whose size follows it, the launch plan of the streams, the
// live counters, the counter rows and the buffer of the small tables.
static int us_buffers(Acquire &q) {
    pbrt_scene *s = q.s;
    pbrt_ctx *c = q.c;
    const bool streams = q.streams;
    int rc;
    // paths in flight per pass.  Streams: 2 x 10 launches per pass whatever is still alive, so passes as large as the radiance
    // streams take (wf_default_pass_paths; the shared trace / shade workspace).  The fused kernels: the pass buffers must fit the
    // context's workspace limit.  A failed allocation halves the pass (size_pass); the echoes do not depend on the pass size.
    q.region = streams ? WF_REGION : us_region_segs(s->accel_kernel, q.rq.emit) * seg_threads(s->accel_kernel);
    const uint64_t pass_paths = default_pass_paths(c, streams, US_PASS_PATHS, 2 * N_STATE * 4);
    // (the fused ultrasound kernels address US_N_STATE dwords per slot of the state tiles)
    if ((rc = size_pass(c, pass_paths, false, q.ppr, q.rq.n_rays, q.region, false, streams, US_N_STATE, UsAllocPass{q}, &q.ps)) != 0) return rc;
    if (streams) {
        q.wfp = wf_plan(s, q.sw);
        q.wfp.packet = false;
        if ((rc = wf_set_attr(s, q.wfp)) != 0) return rc;
    }
    // live counters / statistics rows: per region, per wave of a region for the BVH kernels
    q.n_own = q.ps.nseg * (streams ? WF_SHADE_THREADS / 64u : us_owners_per_region(s->accel_kernel));
    if (!streams) {
        q.segA = (uint32_t *)c->buf("segA", (size_t)q.n_own * 4);
        q.segB = (uint32_t *)c->buf("segB", (size_t)q.n_own * 4);
    }
    // the counter rows: summed into the pinned page and zeroed again by k_us_reduce_stats at the end of the call
    q.segstats_bytes = (size_t)(2 + MAX_DEPTH_STATS) * q.n_own * 8;
    q.segstats = (unsigned long long *)c->buf("us_stats", q.segstats_bytes);
    if (!q.segstats) return PBRT_E_NOMEM;
    q.tabs = (float *)c->buf("us_tables", ((size_t)q.rq.n_rays + 3 * q.rq.NA + q.rq.n_ex) * 4);
    if ((!streams && (!q.segA || !q.segB)) || !q.tabs) return PBRT_E_NOMEM;
    return PBRT_OK;
}

// The three small tables in one host image, uploaded only when they differ from what the device copy already holds, and what the
// call clears: the channel buffer, the counter rows unless they are clean.  (A recording can neither upload nor fill.)
static int us_tables(Acquire &q) {
    pbrt_ctx *c = q.c;
    const UsRequest &rq = q.rq;
    hipStream_t st = c->stream;
    std::vector<float> img((size_t)rq.n_rays + 3 * rq.NA + rq.n_ex);
    float *tx = img.data(), *dir0 = tx + rq.n_rays, *ex = dir0 + 3 * rq.NA;
    pbrt_us_tx_delays(q.p, tx);
    if (q.tx_host) std::memcpy(q.tx_host, tx, (size_t)rq.n_rays * 4);
    if (rq.emit)  // the ray's own emission time rides in its time of flight (CustomEmmitter.py:93-94); t0 of :329 is 0
        std::fill(tx, tx + rq.n_rays, 0.0f);
    std::copy(rq.dir0, rq.dir0 + 3 * rq.NA, dir0);
    if (rq.convex)
        pbrt_us_array_elements(q.p, ex);
    else
        for (uint32_t e = 0; e < rq.NE; ++e) ex[e] = us_elem_x(q.p, e);
    const uint64_t gen = c->work.generation("us_tables");
    if (c->us_tab_gen != gen || c->us_tab_host != img) {
        if (c->recording) return c->fail(PBRT_E_INVALID, "recording: the acquisition's tables are not on the device yet -- run the chain once before recording it");
        c->work.invalidate_recordings();  // (a finished recording was made with the tables that are replaced now)
        HIPCHK(c, hipMemcpyAsync(q.tabs, img.data(), img.size() * 4, hipMemcpyHostToDevice, st));
        c->us_tab_host.swap(img);
        c->us_tab_gen = gen;
    }
    HIPCHK(c, hipMemsetAsync(q.d_channel, 0, rq.nchan * 4, st));
    // (the rows are clean if the last acquisition's reduction has swept exactly this allocation; anything else -- a fresh or resized
    // buffer, a call that failed half-way -- gets the fill)
    if (c->us_rows_gen != c->work.generation("us_stats") || c->us_rows_bytes != q.segstats_bytes) {
        if (c->recording) return c->fail(PBRT_E_INVALID, "recording: the acquisition's counters are not clean yet -- run the chain once before recording it");
        HIPCHK(c, hipMemsetAsync(q.segstats, 0, q.segstats_bytes, st));
    }
    c->us_rows_gen = 0;
    if (q.timed) HIPCHK(c, hipEventRecord(c->ev0, st));
    return PBRT_OK;
}

// Argument block: what every pass hands its kernels, and the first-bounce tables made with it (k_us_first).
static int us_args(Acquire &q) {
    pbrt_scene *s = q.s;
    pbrt_ctx *c = q.c;
    const UsRequest &rq = q.rq;
    const uint32_t NE = rq.NE, n_rays = rq.n_rays;
    UsArgs &a = q.a;
    us_request_args(rq, &a);  // the block with primary without the array bit, tn, am .. inv_c, fuse
    a.sc = s->ds;
    a.stats = q.segstats;
    a.stat_stride = q.n_own;
    a.channel = q.d_channel;
    a.tx = q.tabs;
    a.dir0 = q.tabs + n_rays;
    a.elem_x = q.tabs + n_rays + 3 * rq.NA;
    a.cap = q.ps.cap;
    a.seed = q.seed;
    a.lds_bytes = s->lds_bytes;
    a.div_ne = make_fastdiv(NE);
    NEED(c, fastdiv_exact(a.div_ne, NE, {0u, 1u, NE - 1, NE, NE + 1, n_rays - 1, n_rays}));
    if (rq.tables) {
        float4 *fh = (float4 *)c->buf("us_first_hit", (size_t)n_rays * 16);
        float4 *fv = (float4 *)c->buf("us_first_rx", (size_t)n_rays * NE * 16);
        if (!fh || !fv) return PBRT_E_NOMEM;
        const dim3 g(div_up((uint64_t)n_rays * NE, 256)), b(256);
        hipLaunchKernelGGL(us_first_kernel(s, rq.convex), g, b, 0, c->stream, a, n_rays, fh, fv);
        HIPCHK(c, hipGetLastError());
        a.first_hit = fh;
        a.first_rx = fv;
    }
    return PBRT_OK;
}

// Brute-force scenes: the bounces of one ultrasound pass through the fused k_us_bounce, in one launch (a.fuse) or one per bounce.
// Emitter rays are drawn inside the first-bounce instance (the EMIT instances of k_us_bounce: 17.1 against 18.4 ms since the echo table
// grew); PBRT_US_EMIT_FUSED=0 (A/B, test) writes them into the path state first (k_us_emit_init) and walks every bounce with the
// later-bounce instance.  (Two default bench runs of this form showed steps of 38 - 43 ms; host stalls of that size hit the
// two-kernel form as well and went away when bench.py took Python's cyclic collector out of its timed steps: three runs of
// either form clean since.)
static int us_fused_pass(Acquire &q, uint32_t nseg_pass) {
    pbrt_ctx *c = q.c;
    UsArgs &a = q.a;
    int rc;
    float *in = q.stA, *out = q.stB;
    uint32_t *sin = q.segA, *sout = q.segB;
    // step 0 of the two-kernel form: the primary rays into the state (k_us_emit_init writes a.out / a.seg_out), then the later-bounce
    // instance from depth 0
    const bool emit_init = q.rq.emit && !q.sw.us_emit_fused;
    for (uint32_t depth = 0, step = 0; depth < q.p->max_depth; ++step) {
        a.depth = depth;
        a.in = in;
        a.out = out;
        a.seg_in = sin;
        a.seg_out = sout;
        if (emit_init && step == 0) {
            hipLaunchKernelGGL(k_us_emit_init, dim3(div_up(std::max(a.n_paths, nseg_pass), 256)), dim3(256), 0, c->stream, a, q.region, nseg_pass);
        } else {
            if ((rc = launch_us(q.s, a, nseg_pass, step == 0, q.sw.us_generic_kernel, q.rq.convex)) != 0) return rc;
            HIPCHK(c, hipGetLastError());
            ++q.launches;
            if (a.fuse) break;  // that launch walked every bounce (kernels_us.h)
            ++depth;
        }
        std::swap(in, out);
        std::swap(sin, sout);
    }
    return PBRT_OK;
}

// The pass loop: the paths of a ray in passes of ps.per_pass, each between the events of its own pair.
static int us_passes(Acquire &q) {
    pbrt_ctx *c = q.c;
    UsArgs &a = q.a;
    const uint32_t n_rays = q.rq.n_rays;
    int rc;
    q.timer = PassTimer{c, q.timed};
    for (uint32_t k0 = 0; k0 < q.ppr; k0 += q.ps.per_pass, ++q.passes) {
        const uint32_t kc = std::min(q.ps.per_pass, q.ppr - k0);
        a.ppr_pass = kc;
        a.div_ppr = make_fastdiv(kc);
        NEED(c, fastdiv_exact(a.div_ppr, kc, {0u, 1u, kc - 1, kc, kc + 1, n_rays * kc - 1, n_rays * kc, 0xfffffbffu}));
        a.path_first = q.path_offset + k0;
        a.n_paths = n_rays * kc;
        const uint32_t nseg_pass = div_up(a.n_paths, q.region);
        a.blk_mul = q.rq.emit && !q.streams ? us_emit_blk_mul(nseg_pass, q.rq.NA, q.sw.us_emit_permute) : 0u;
        if ((rc = q.timer.begin()) != 0) return rc;
        rc = q.streams ? us_wf_pass(q.s, a, q.wfb, q.wfp, nseg_pass, q.rq.convex, &q.launches) : us_fused_pass(q, nseg_pass);
        if (rc != 0) return rc;
        if ((rc = q.timer.end()) != 0) return rc;
    }
    return PBRT_OK;
}

// The end of the queued chain: normalisation, the counters into the context's pinned page, and what us_finish needs to turn them
// into pbrt_stats once the stream has drained.
static int us_queue_finish(Acquire &q) {
    pbrt_ctx *c = q.c;
    hipStream_t st = c->stream;
    const uint64_t nchan = q.rq.nchan;
    const float inv_norm = 1.0f / (float)(q.norm_paths ? q.norm_paths : 1);
    // (one path per ray, the reference's own setting (USMain.py:36): the factor is exactly 1 and the pass over the buffer changes no bit)
    if (inv_norm != 1.0f) hipLaunchKernelGGL(k_scale, dim3(div_up(nchan, 256)), dim3(256), 0, st, q.d_channel, nchan, inv_norm);
    HIPCHK(c, hipGetLastError());
    if (q.timed) HIPCHK(c, hipEventRecord(c->ev1, st));
    // counters into the context's pinned page (partial sums, written by the kernel; the rows are zero again behind it), guard words by
    // a queued copy; both are read by us_finish once the stream has drained
    hipLaunchKernelGGL(k_us_reduce_stats, dim3(2 + MAX_DEPTH_STATS, REDUCE_SLICES), dim3(256), 0, st, q.segstats, q.n_own, (size_t)q.n_own, c->pin_stats());
    HIPCHK(c, hipGetLastError());
    c->us_rows_gen = c->work.generation("us_stats");
    c->us_rows_bytes = q.segstats_bytes;
    if (int rc = q.streams ? wf_guard_fetch(c, c->pin_guard()) : PBRT_OK) return rc;
    pbrt_ctx::PendingAcq &P = c->pend;
    P.active = true;
    P.timed = q.timed;
    P.scaled = inv_norm != 1.0f;
    P.streams = q.streams;
    P.tab0 = q.a.first_hit != nullptr;
    P.n_ev = q.timer.n_ev;
    P.passes = q.passes;
    P.launches = q.launches;
    P.samples = (uint64_t)q.rq.n_rays * q.ppr;
    P.nchan = nchan;
    return PBRT_OK;
}

static int us_impl(pbrt_scene *s, const pbrt_us_params *p, uint32_t seed, uint32_t ppr, uint32_t path_offset,
                   uint32_t norm_paths, float *d_channel, float *tx_host, bool wait = true) {
    Acquire q{s, s->ctx, p, seed, ppr, path_offset, norm_paths, d_channel, tx_host, wait};
    for (auto stage : {us_check, us_buffers, us_tables, us_args, us_passes, us_queue_finish})
        if (int rc = stage(q)) return rc;
    return wait ? us_finish(q.c) : PBRT_OK;
}

static int us_finish(pbrt_ctx *c) {
    pbrt_ctx::PendingAcq P = c->pend;
    c->pend.active = false;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIPCHK(c, hipStreamSynchronize(st));
    int rc;
    if (P.streams && (rc = wf_check_guard(c, c->pin_guard())) != 0) return rc;
    unsigned long long hstats[2 + MAX_DEPTH_STATS];  // the slices of a row, added here
    for (uint32_t r = 0; r < 2 + MAX_DEPTH_STATS; ++r) {
        unsigned long long t = 0;
        for (uint32_t sl = 0; sl < REDUCE_SLICES; ++sl) t += c->pin_stats()[(size_t)r * REDUCE_SLICES + sl];
        hstats[r] = t;
    }
    if ((rc = call_stats(c, hstats, P.samples, P.launches, P.passes, P.timed, P.n_ev)) != 0) return rc;
    pbrt_stats &S = c->stats;
    uint64_t bb = 0;
    for (uint32_t d = 0; d < MAX_DEPTH_STATS; ++d) {
        uint64_t in = hstats[2 + d], next = d + 1 < MAX_DEPTH_STATS ? hstats[2 + d + 1] : 0;
        if (d > 0) bb += in * (N_USTATE * 4);
        bb += next * (N_USTATE * 4);
    }
    bb += hstats[0] * 8;  // one f32 atomic (read-modify-write) per shaded segment, upper bound
    if (P.streams) {
        // k_trace + k_us_shade (kernels_us_wavefront.h), the bytes the algorithm needs: per ray that is traced 32 B read + 4 B hit
        // index written and read back; a path's pending echo (32 B) is read once,
        // the rest of its state (32 B) if it hit; 64 B per survivor; an occlusion ray is 32 B written, 32 B read, 4 B answered.
        // (With the first-bounce tables depth 0 traces and reads nothing.)  Occlusion rays: one per shaded segment at most.
        const bool tab0 = P.tab0;
        uint64_t tr = 0, sh = 0;
        for (uint32_t d = 0; d < MAX_DEPTH_STATS; ++d) {
            const uint64_t in = hstats[2 + d], next = d + 1 < MAX_DEPTH_STATS ? hstats[2 + d + 1] : 0;
            if (!in) break;
            if (d > 0 || !tab0) {
                tr += in * (32 + 4);
                sh += in * (4 + 32);
            }
            sh += next * 64;
        }
        const uint64_t seg = hstats[0], seg_traced = tab0 ? seg - std::min<uint64_t>(seg, hstats[2]) : seg;  // (every path of depth 0 hits or none of its ray does)
        tr += seg_traced * 36;
        sh += seg_traced * (32 + 32) + seg * 8;
        bb = tr + sh;
        S.trace_model_bytes = tr;
    }
    S.bounce_model_bytes = bb;
    S.model_bytes = bb + P.nchan * (P.scaled ? 12 : 4);  // clear (+ scale pass) over the channel buffer
    return PBRT_OK;
}

extern "C" {

int pbrt_us_acquire_dev(pbrt_scene *s, const pbrt_us_params *p, uint32_t seed, uint32_t ppr, uint32_t path_offset,
                        uint32_t norm_paths, void *d_channel, float *tx) {
    if (!s) return PBRT_E_INVALID;
    ++s->ctx->call_seq;
    return us_impl(s, p, seed, ppr, path_offset, norm_paths, (float *)d_channel, tx);
}

int pbrt_us_acquire_queue_dev(pbrt_scene *s, const pbrt_us_params *p, uint32_t seed, uint32_t ppr, uint32_t path_offset,
                              uint32_t norm_paths, void *d_channel, float *tx) {
    if (!s) return PBRT_E_INVALID;
    ++s->ctx->call_seq;
    return us_impl(s, p, seed, ppr, path_offset, norm_paths, (float *)d_channel, tx, false);
}

int pbrt_us_acquire(pbrt_scene *s, const pbrt_us_params *p, uint32_t seed, uint32_t ppr, uint32_t path_offset,
                    uint32_t norm_paths, float *channel, float *tx) {
    if (!s) return PBRT_E_INVALID;
    pbrt_ctx *c = s->ctx;
    NEED(c, p && channel);
    HIPCHK(c, hipSetDevice(c->device));
    ++c->call_seq;
    const size_t n = (size_t)p->n_angles * p->n_elements * p->time_samples;
    void *d = c->buf("us_channel", n * 4);
    if (!d) return PBRT_E_NOMEM;
    int rc = us_impl(s, p, seed, ppr, path_offset, norm_paths, (float *)d, tx);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(channel, d, n * 4, hipMemcpyDeviceToHost));
    return PBRT_OK;
}

// ------------------------------------------------------------------------------------------------
// leaf operators: stage host SoA through the workspace, one kernel, copy back
// ------------------------------------------------------------------------------------------------
}  // extern "C"

// The staging area of one call (stage_layout.h): arrays() takes the call's arrays, each named once, asks the workspace for what their
// layout needs, uploads the inputs and returns the device pointers; finish() downloads the outputs and waits (both in argument order)
struct Stage {
    pbrt_ctx *c;
    int rc = PBRT_OK;  // looked at after arrays(): PBRT_E_NOMEM, or a failed upload
    struct Back { void *h; const void *d; size_t bytes; } backs[16] = {};  // the outputs, for finish()
    size_t n_back = 0;
    template <class... T>
    std::tuple<T *...> arrays(const StageArray<T> &...a) {
        static_assert(sizeof...(T) <= sizeof(backs) / sizeof(backs[0]), "more arrays than a staged call can download");
        const auto L = stage_layout(a...);
        ++c->call_seq;
        char *base = (char *)c->buf("leaf_io", L.total);
        if (!base) rc = PBRT_E_NOMEM;
        size_t i = 0;
        return std::tuple<T *...>{place(base, L.offset[i++], a)...};  // (a braced list: evaluated left to right)
    }
    template <class T>
    T *place(char *base, size_t off, const StageArray<T> &a) {
        if (!base || (a.input && !a.src)) return nullptr;
        T *d = reinterpret_cast<T *>(base + off);
        if (a.input && rc == PBRT_OK && hipMemcpyAsync(d, a.src, a.bytes(), hipMemcpyHostToDevice, c->stream) != hipSuccess)
            rc = c->fail(PBRT_E_DEVICE, "leaf upload failed");
        if (a.dst) backs[n_back++] = Back{a.dst, d, a.bytes()};
        return d;
    }
    int finish() {
        for (size_t i = 0; i < n_back && rc == PBRT_OK; ++i)
            if (hipMemcpyAsync(backs[i].h, backs[i].d, backs[i].bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
                rc = c->fail(PBRT_E_DEVICE, "leaf download failed");
        if (rc != PBRT_OK) return rc;
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return c->fail(PBRT_E_DEVICE, "leaf kernel: %s", hipGetErrorString(e));
        return PBRT_OK;
    }
};

extern "C" {

// entering a call that stages host arrays through the workspace (`empty`: it has nothing to do): declares S
#define STAGED_BEGIN(c, empty)             \
    if (empty) return PBRT_OK;             \
    NOT_RECORDING(c);                      \
    HIPCHK(c, hipSetDevice((c)->device));  \
    Stage S{c}
// the rest of a staged call: nothing more if S.arrays() failed, the queueing function (its failure returns before any download or wait), finish()
#define STAGED_RUN(S, enqueue)               \
    if ((S).rc) return (S).rc;               \
    if (int rc_ = (enqueue)) return rc_;     \
    return (S).finish()
// the same for a leaf operator on n items: its launch is one thread per item
#define LEAF_RUN(S, n, kernel, ...)                                                                              \
    if ((S).rc) return (S).rc;                                                                                   \
    hipLaunchKernelGGL(kernel, dim3(div_up(n, 256)), dim3(256), 0, (S).c->stream, __VA_ARGS__);                  \
    return (S).finish()

int pbrt_ray_intersect(pbrt_scene *s, uint32_t n, const float *o, const float *d, const float *tmax, float *t,
                       uint32_t *prim, float *u, float *v) {
    if (!s) return PBRT_E_INVALID;
    NEED(s->ctx, o && d && tmax && t && prim && u && v);
    STAGED_BEGIN(s->ctx, n == 0);
    auto [dO, dD, dT, rt, rp, ru, rv] = S.arrays(stage_in(o, 3 * (size_t)n), stage_in(d, 3 * (size_t)n), stage_in(tmax, n), stage_out(t, n),
                                                 stage_out(prim, n), stage_out(u, n), stage_out(v, n));
    LEAF_RUN(S, n, ray_intersect_kernel(s), s->ds, n, dO, dD, dT, rt, rp, ru, rv);
}

int pbrt_ray_test(pbrt_scene *s, uint32_t n, const float *o, const float *d, const float *tmax, uint8_t *hit) {
    if (!s) return PBRT_E_INVALID;
    NEED(s->ctx, o && d && tmax && hit);
    STAGED_BEGIN(s->ctx, n == 0);
    auto [dO, dD, dT, rh] = S.arrays(stage_in(o, 3 * (size_t)n), stage_in(d, 3 * (size_t)n), stage_in(tmax, n), stage_out(hit, n));
    LEAF_RUN(S, n, ray_test_kernel(s), s->ds, n, dO, dD, dT, rh);
}

int pbrt_bsdf_sample(pbrt_ctx *ctx, const pbrt_material *m, uint32_t quirks, uint32_t n, const float *wi,
                     const float *n_geo, const float *n_sh, const float *sh_s, const float *s1, const float *s2, float *wo,
                     float *pdf, float *weight, uint32_t *sampled) {
    if (!ctx) return PBRT_E_INVALID;
    NEED(ctx, m && wi && s1 && s2 && wo && pdf && weight && sampled);
    MATERIAL_RULE(ctx, *m, 0);
    STAGED_BEGIN(ctx, n == 0);
    const size_t n3 = 3 * (size_t)n;  // (n_geo, n_sh, sh_s may be null: the slot stays, the kernel gets a null pointer)
    auto [dwi, dng, dns, dss, d1, d2, rwo, rpdf, rw, rs] =
        S.arrays(stage_in(wi, n3), stage_in(n_geo, n3), stage_in(n_sh, n3), stage_in(sh_s, n3), stage_in(s1, n), stage_in(s2, 2 * (size_t)n),
                 stage_out(wo, n3), stage_out(pdf, n), stage_out(weight, n3), stage_out(sampled, n));
    LEAF_RUN(S, n, k_bsdf_sample, *m, quirks, n, dwi, dng, dns, dss, d1, d2, rwo, rpdf, rw, rs);
}

int pbrt_bsdf_eval_pdf(pbrt_ctx *ctx, const pbrt_material *m, uint32_t n, const float *wi, const float *wo, float *f,
                       float *pdf) {
    if (!ctx) return PBRT_E_INVALID;
    NEED(ctx, m && wi && wo && f && pdf);
    MATERIAL_RULE(ctx, *m, 0);
    STAGED_BEGIN(ctx, n == 0);
    const size_t n3 = 3 * (size_t)n;
    auto [dwi, dwo, rf, rp] = S.arrays(stage_in(wi, n3), stage_in(wo, n3), stage_out(f, n3), stage_out(pdf, n));
    LEAF_RUN(S, n, k_bsdf_eval_pdf, *m, n, dwi, dwo, rf, rp);
}

int pbrt_emitter_sample_direction(pbrt_scene *s, uint32_t n, const float *p, const float *u, float *d, float *dist,
                                  float *pdf, float *weight, float *q, uint32_t *emitter) {
    if (!s) return PBRT_E_INVALID;
    NEED(s->ctx, p && u && d && dist && pdf && weight && q && emitter);
    STAGED_BEGIN(s->ctx, n == 0);
    const size_t n3 = 3 * (size_t)n;
    auto [dp, du, rd, rdist, rpdf, rw, rq, re] = S.arrays(stage_in(p, n3), stage_in(u, 4 * (size_t)n), stage_out(d, n3), stage_out(dist, n),
                                                          stage_out(pdf, n), stage_out(weight, n3), stage_out(q, n3), stage_out(emitter, n));
    LEAF_RUN(S, n, k_emitter_sample, s->ds, n, dp, du, rd, rdist, rpdf, rw, rq, re);
}

int pbrt_sensor_sample_ray(pbrt_ctx *ctx, const pbrt_camera *cam, uint32_t n, const float *pos, float *o, float *d,
                           float *tmax) {
    if (!ctx) return PBRT_E_INVALID;
    NEED(ctx, cam && pos && o && d && tmax);
    STAGED_BEGIN(ctx, n == 0);
    auto [dp, ro, rd, rt] = S.arrays(stage_in(pos, 2 * (size_t)n), stage_out(o, 3 * (size_t)n), stage_out(d, 3 * (size_t)n), stage_out(tmax, n));
    LEAF_RUN(S, n, k_sensor_sample_ray, *cam, n, dp, ro, rd, rt);
}

int pbrt_us_sensor_sample_ray(pbrt_ctx *ctx, const pbrt_us_sensor *sn, int use_hemisphere_warp, uint32_t n,
                              const float *time, const float *wavelength_sample, const float *position_sample,
                              const float *aperture_sample, float *o, float *d, float *weight) {
    if (!ctx) return PBRT_E_INVALID;
    NEED(ctx, sn && time && wavelength_sample && position_sample && aperture_sample && o && d && weight);
    STAGED_BEGIN(ctx, n == 0);
    auto [dt, dw, dp, da, ro, rd, rw] =
        S.arrays(stage_in(time, n), stage_in(wavelength_sample, n), stage_in(position_sample, 2 * (size_t)n),
                 stage_in(aperture_sample, 2 * (size_t)n), stage_out(o, 3 * (size_t)n), stage_out(d, 3 * (size_t)n), stage_out(weight, n));
    LEAF_RUN(S, n, k_us_sensor_sample_ray, *sn, use_hemisphere_warp, n, dt, dw, dp, da, ro, rd, rw);
}

int pbrt_us_emitter_sample_ray(pbrt_ctx *ctx, const pbrt_us_emitter *e, uint32_t n, const float *time, const float *s1,
                               const float *s2, const float *s3, float *o, float *d, float *ray_time, float *weight,
                               float *pdf_pos) {
    if (!ctx) return PBRT_E_INVALID;
    NEED(ctx, e && time && s1 && s2 && s3 && o && d && ray_time && weight && pdf_pos);
    STAGED_BEGIN(ctx, n == 0);
    auto [dt, d1, d2, d3, ro, rd, rt, rw, rp] =
        S.arrays(stage_in(time, n), stage_in(s1, n), stage_in(s2, 2 * (size_t)n), stage_in(s3, n), stage_out(o, 3 * (size_t)n),
                 stage_out(d, 3 * (size_t)n), stage_out(ray_time, n), stage_out(weight, n), stage_out(pdf_pos, n));
    LEAF_RUN(S, n, k_us_emitter_sample_ray, *e, n, dt, d1, d2, d3, ro, rd, rt, rw, rp);
}

int pbrt_us_put_data(pbrt_ctx *ctx, const pbrt_us_receiver *r, uint32_t n, const float *ox, const float *time,
                     const float *d, const float *amplitude, float *channel_buffer) {
    if (!ctx) return PBRT_E_INVALID;
    NEED(ctx, r && ox && time && d && amplitude && channel_buffer);
    STAGED_BEGIN(ctx, n == 0);
    auto [dx, dt, dd, da, db] = S.arrays(stage_in(ox, n), stage_in(time, n), stage_in(d, 3 * (size_t)n), stage_in(amplitude, n),
                                         stage_inout(channel_buffer, (size_t)r->number_of_elements * r->time_samples));
    LEAF_RUN(S, n, k_us_put_data, *r, n, dx, dt, dd, da, db);
}

// ------------------------------------------------------------------------------------------------
// image formation behind the hot path: (pulse ->) beamform -> envelope -> log compression.
// The *_dev entry points queue their kernels on the context's stream and return (ABI 5): the reference's us_render loop
// (USMain.py:92-252, 51 x per run) stays in HBM from the acquisition to the display image.  The host-pointer forms stage
// their arguments and call the same queueing functions.  The rules of the seven steps around the beamformer, what makes a call of theirs
// empty and the shape of every launch are in img_request.h (host only): an entry point makes its request, *_enqueue adds what needs the device.
// ------------------------------------------------------------------------------------------------
}  // extern "C"

// an event pair around one image-formation step when the context profiles (pbrt_ctx_set_profiling); slot = IMG_*
enum { IMG_PULSE = 0, IMG_DAS = 1, IMG_ENV = 2, IMG_LOG = 3, IMG_STEPS = 4 };
struct ImgTimer {
    pbrt_ctx *c;
    int slot;
    ImgTimer(pbrt_ctx *ctx, int s) : c(ctx), slot(s) {
        if (c->profiling && !c->recording && c->img_event(2 * slot)) (void)hipEventRecord(c->img_ev[2 * slot], c->stream);
    }
    ~ImgTimer() {
        if (c->profiling && !c->recording && c->img_event(2 * slot + 1)) {
            (void)hipEventRecord(c->img_ev[2 * slot + 1], c->stream);
            c->img_mask |= 1u << slot;
        }
    }
};

static int launched(pbrt_ctx *c) {  // the end of every function that queues kernels
    HIPCHK(c, hipGetLastError());
    return PBRT_OK;
}
// ---- one beamform request (bf_request.h: the request, and the rules of the four parameter blocks) from the entry points to the launch ----
// de: element positions [n_elements], or (rq.probe) the element table [n_elements][4]; dx, dz: the axes, or (rq.tab) the pixel tables;
// dt, ttx: the transmit delays, and the first-arrival table of this scan or null
// DAS_PICK(k<I, T, X ...>): the selector of a beamform family for with_flags(linear interpolation, first-arrival table, element table)
#define DAS_PICK(...)                                                                    \
    [](auto L, auto Tab, auto Probe) {                                                   \
        constexpr uint32_t I = L() ? PBRT_DAS_LINEAR : PBRT_DAS_NEAREST;                 \
        constexpr bool T = Tab(), X = Probe();                                           \
        return &__VA_ARGS__;                                                             \
    }
static int das_enqueue(pbrt_ctx *c, const BfRequest &rq, const float *dd, const float *dt, const float *de, const float *dx, const float *dz,
                       float *dout, const double *ttx, const CaponRequest *capon = nullptr, const CoherenceRequest *coh = nullptr) {
    const pbrt_das_params *p = rq.das;
    int rc = PBRT_OK;
    ImgTimer tm(c, IMG_DAS);
    DasGrid g;
    const uint32_t blocks = das_grid(&g, p->nx, p->nz, rq.tab);
    // The one launch: `pick` names a family's instance for <INTERP, TABLE, CONVEX>, the nine arguments every family takes follow (the
    // samples and the pixels as the method's type, kernels_beamform.h DasSample), then the family's own.
    const auto family = [&](auto method) {
        constexpr uint32_t M = decltype(method)::value;
        typedef typename DasSample<M>::type Sample;
        const auto launch_lds = [&](size_t lds, auto pick, auto... own) {  // lds: the dynamic LDS of the launch
            const auto kernel = with_flags(pick, p->interpolation != PBRT_DAS_NEAREST, ttx != nullptr, rq.probe);
            if (const hipError_t e = coh_allow_lds(kernel, lds); e != hipSuccess)
                return (void)(rc = c->fail(PBRT_E_DEVICE, "hipFuncSetAttribute(k_coherence_beamform, %zu bytes of LDS): %s", lds, hipGetErrorString(e)));
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * DAS_SPLIT), lds, c->stream, *p, g, reinterpret_cast<const Sample *>(dd), dt, de, dx,
                               dz, ttx, reinterpret_cast<Sample *>(dout), own...);
        };
        const auto launch = [&](auto pick, auto... own) { launch_lds(0, pick, own...); };
        //  the request                                    its kernel                              the kernel's own arguments
        if constexpr (M == BF_IQ) {  // (Capon's samples are I/Q pairs: the switch below sends every Capon request here)
            if (capon)                              return launch(DAS_PICK(k_capon_beamform<I, T, X>),    rq.pw, capon->l_prop, capon->delta_l);  // (D23)
            if (coh && coh->kind == PBRT_COH_SLSC)  return launch_lds(coh->lds_bytes, DAS_PICK(k_coherence_beamform<I, T, X, PBRT_COH_SLSC>), rq.pw, coh->lag_prop, coh->half_kernel);  // (D26)
            if (coh)                                return launch_lds(coh->lds_bytes, DAS_PICK(k_coherence_beamform<I, T, X, PBRT_COH_CF>),   rq.pw, coh->gamma, coh->half_kernel);
        }
        if (rq.window != PBRT_APOD_BOXCAR)          return launch(DAS_PICK(k_apod_beamform<I, T, X, M>),  rq.pw, rq.a0, rq.alpha);                // (D22)
        if constexpr (M == BF_IQ)                   return launch(DAS_PICK(k_iq_beamform<I, T, X>),       rq.pw);  // pw: the demodulation frequency
        else if constexpr (M == BF_DAS)             return launch(DAS_PICK(k_das_beamform<I, T, X>));
        else                                        return launch(DAS_PICK(k_nl_beamform<I, T, X, M>),    rq.pw);  // pw: p
    };
    // (bf_request admits four methods and capon_request I/Q alone; what they would refuse goes where it went before this table was one:
    // a Capon request to Capon whatever its method, an unknown method to p-DAS)
    switch (capon || coh ? (uint32_t)PBRT_SCAN_IQ : rq.method) {
        case PBRT_SCAN_IQ: family(std::integral_constant<uint32_t, BF_IQ>{}); break;
        case PBRT_BF_FDMAS: family(std::integral_constant<uint32_t, PBRT_BF_FDMAS>{}); break;
        default: family(std::integral_constant<uint32_t, PBRT_BF_PDAS>{}); break;
        case PBRT_SCAN_DAS: family(std::integral_constant<uint32_t, BF_DAS>{}); break;
    }
    if (rc != PBRT_OK) return rc;
    c->img_das_bytes = ((uint64_t)p->n_angles * p->n_elements * p->time_samples + (uint64_t)p->nx * p->nz) * (rq.method == PBRT_SCAN_IQ ? 8 : 4);
    return launched(c);
}
// the launch of an image step as its request shapes it (img_request.h ImgLaunch: grid, block, dynamic LDS bytes)
#define IMG_LAUNCH(c, L, kernel, ...) hipLaunchKernelGGL(kernel, dim3((L).gx, (L).gy), dim3((L).block), (L).lds, (c)->stream, __VA_ARGS__)

static int env_enqueue(pbrt_ctx *c, const EnvRequest &rq, const float *din, float *dout) {
    // the tap table of this column length: made once, kept while the workspace buffer lives (pbrt_ctx_trim may take it)
    float *taps = (float *)c->buf("env_taps", (size_t)ENV_TAPS_FLOATS * 4);
    if (!taps) return PBRT_E_NOMEM;
    const uint64_t gen = c->work.generation("env_taps");
    ImgTimer tm(c, IMG_ENV);
    if (gen != c->env_taps_gen || c->env_taps_n != rq.nz) {
        c->work.invalidate_recordings();  // (a finished recording holds no launch of this kernel: its taps are replaced now)
        IMG_LAUNCH(c, rq.taps_launch, k_hilbert_taps, rq.nz, taps);
        c->env_taps_n = rq.nz;
        c->env_taps_gen = gen;
    }
    if (const size_t lds = rq.launch.lds; lds > c->env_lds_attr) {
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_hilbert_env), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_hilbert_env_even), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        c->env_lds_attr = lds;
    }
    IMG_LAUNCH(c, rq.launch, rq.even ? k_hilbert_env_even : k_hilbert_env, rq.nz, din, taps, dout);
    return launched(c);
}
static int log_enqueue(pbrt_ctx *c, const LogRequest &rq, const float *din, float *dout) {
    float *mx = (float *)c->buf("img_max", ENV_MAX_BLOCKS * 4);
    if (!mx) return PBRT_E_NOMEM;
    ImgTimer tm(c, IMG_LOG);
    IMG_LAUNCH(c, rq.max_launch, k_env_max, rq.n, din, mx);
    IMG_LAUNCH(c, rq.launch, k_log_compress, rq.n, din, mx, rq.nb, rq.dynamic_range_db, dout);
    return launched(c);
}
static int pulse_enqueue(pbrt_ctx *c, const PulseRequest &rq, const float *din, float *dout) {
    ImgTimer tm(c, IMG_PULSE);
    IMG_LAUNCH(c, rq.launch, k_apply_pulse, rq.T, rq.K, rq.fs, rq.frequency, rq.sigma, din, dout);
    return launched(c);
}
static int fir_enqueue(pbrt_ctx *c, const FirRequest &rq, const float *dtaps, const float *din, float *dout) {
    IMG_LAUNCH(c, rq.launch, k_axial_fir, rq.nz, rq.K, rq.per_col, dtaps, din, dout);
    return launched(c);
}
static int scan_convert_enqueue(pbrt_ctx *c, const ScanConvertRequest &rq, const float *dsrc, const float *dx, const float *dz, float *ddst) {
    IMG_LAUNCH(c, rq.launch, k_scan_convert, *rq.p, dsrc, dx, dz, ddst);
    return launched(c);
}
static int rf2iq_enqueue(pbrt_ctx *c, const Rf2iqRequest &rq, const float *dtaps, const float *din, float *dout) {
    IMG_LAUNCH(c, rq.launch, k_rf2iq, rq.T, rq.Td, rq.K, rq.D, rq.per_trace, rq.fs, rq.t0, rq.demod_freq, dtaps, din,
               reinterpret_cast<float2 *>(dout));
    return launched(c);
}
static int iq_env_enqueue(pbrt_ctx *c, const IqEnvRequest &rq, const float *din, float *dout) {
    ImgTimer tm(c, IMG_ENV);
    IMG_LAUNCH(c, rq.launch, k_iq_modulus, rq.n, reinterpret_cast<const float2 *>(din), dout);
    return launched(c);
}

// The three bodies behind the 26 beamform and first-arrival entry points (capon / coh: the request of pbrt_capon_* / pbrt_coherence_*, else null).  Each entry point makes its request first (BF_REQUEST below):
// a null context is PBRT_E_INVALID and touches nothing, a refused block is PBRT_E_INVALID with the text of the rule.
// (d_tx_delays or d_table: the plain form passes its delays, the table form its first-arrival table, and the other one null)
static int beamform_dev(pbrt_ctx *ctx, const BfRequest &rq, const void *d_data, const void *d_elem, const void *d_x, const void *d_z,
                        void *d_out, const void *d_tx_delays, const void *d_table, const CaponRequest *capon = nullptr, const CoherenceRequest *coh = nullptr) {
    NEED(ctx, d_data && (d_tx_delays || d_table) && d_elem && d_x && d_z && d_out);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return das_enqueue(ctx, rq, (const float *)d_data, (const float *)d_tx_delays, (const float *)d_elem, (const float *)d_x,
                       (const float *)d_z, (float *)d_out, (const double *)d_table, capon, coh);
}

static int first_arrival_dev(pbrt_ctx *ctx, const BfRequest &rq, const void *d_tx_delays, const void *d_elem, const void *d_x, const void *d_z,
                             void *d_table) {
    NEED(ctx, d_tx_delays && d_elem && d_x && d_z && d_table);
    const pbrt_das_params *p = rq.das;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(rq.probe ? k_das_first_arrival<true> : k_das_first_arrival<false>, dim3(div_up((uint64_t)p->nx * p->nz, 256)), dim3(256),
                       0, ctx->stream, *p, rq.tab ? 1u : 0u, (const float *)d_tx_delays, (const float *)d_elem, (const float *)d_x,
                       (const float *)d_z, (double *)d_table);
    return launched(ctx);
}

static int beamform_host(pbrt_ctx *ctx, const BfRequest &rq, const float *data, const float *tx_delays, const float *elem, const float *x,
                         const float *z, float *out, const CaponRequest *capon = nullptr, const CoherenceRequest *coh = nullptr) {
    NEED(ctx, data && tx_delays && elem && x && z && out);
    const pbrt_das_params *p = rq.das;
    const size_t width = rq.method == PBRT_SCAN_IQ ? 2u : 1u, out_width = coh ? coh->width : width;  // floats per sample, and per pixel (an SLSC image is real)
    const size_t nd = (size_t)p->n_angles * p->n_elements * p->time_samples * width, ne = (size_t)p->n_angles * p->n_elements;
    const uint32_t n = p->nx * p->nz;
    const size_t nel = (size_t)p->n_elements * (rq.probe ? 4u : 1u);
    const size_t ngx = rq.tab ? (size_t)n : p->nx, ngz = rq.tab ? (size_t)n : p->nz;  // axes, or the two pixel tables
    STAGED_BEGIN(ctx, n == 0);
    auto [dd, dt, de, dx, dz, dout] =
        S.arrays(stage_in(data, nd), stage_in(tx_delays, ne), stage_in(elem, nel), stage_in(x, ngx), stage_in(z, ngz), stage_out(out, n * out_width));
    STAGED_RUN(S, das_enqueue(ctx, rq, dd, dt, de, dx, dz, dout, nullptr, capon, coh));
}
// entering an entry point of the image chain: declares rq, the request its maker fills (bf_request.h, img_request.h)
#define MAKE_REQUEST(ctx, Request, maker, ...) \
    Request rq;                                \
    if (!(ctx)) return PBRT_E_INVALID;         \
    if (const char *why = maker(&rq, __VA_ARGS__)) return (ctx)->fail(PBRT_E_INVALID, "invalid argument: %s", why)
#define BF_REQUEST(...) MAKE_REQUEST(ctx, BfRequest, bf_request, __VA_ARGS__)
// The two sequences of the fourteen image-step entry points, each stated once.  A _dev form: null context -> request -> refused ->
// empty -> hipSetDevice, then it queues.  A host form: ... -> empty -> not while recording -> hipSetDevice (STAGED_BEGIN, which
// declares S), then it stages, queues, downloads and waits (STAGED_RUN).
#define IMG_QUEUED(ctx, Request, maker, ...)        \
    MAKE_REQUEST(ctx, Request, maker, __VA_ARGS__); \
    if (rq.empty) return PBRT_OK;                   \
    HIPCHK(ctx, hipSetDevice((ctx)->device))
#define IMG_STAGED(ctx, Request, maker, ...)        \
    MAKE_REQUEST(ctx, Request, maker, __VA_ARGS__); \
    STAGED_BEGIN(ctx, rq.empty)

extern "C" {

int pbrt_scan_beamform(pbrt_ctx *ctx, const pbrt_scan_params *p, const float *data, const float *tx_delays, const float *elem,
                       const float *px, const float *pz, float *out) {
    BF_REQUEST(p);
    return beamform_host(ctx, rq, data, tx_delays, elem, px, pz, out);
}
int pbrt_scan_beamform_dev(pbrt_ctx *ctx, const pbrt_scan_params *p, const void *d_data, const void *d_tx_delays, const void *d_elem,
                           const void *d_px, const void *d_pz, void *d_out) {
    BF_REQUEST(p);
    return beamform_dev(ctx, rq, d_data, d_elem, d_px, d_pz, d_out, d_tx_delays, nullptr);
}
int pbrt_scan_beamform_table_dev(pbrt_ctx *ctx, const pbrt_scan_params *p, const void *d_data, const void *d_table, const void *d_elem,
                                 const void *d_px, const void *d_pz, void *d_out) {
    BF_REQUEST(p);
    return beamform_dev(ctx, rq, d_data, d_elem, d_px, d_pz, d_out, nullptr, d_table);
}
int pbrt_apod_beamform(pbrt_ctx *ctx, const pbrt_apod_params *p, const float *data, const float *tx_delays, const float *elem,
                       const float *px, const float *pz, float *out) {
    BF_REQUEST(p);
    return beamform_host(ctx, rq, data, tx_delays, elem, px, pz, out);
}
int pbrt_apod_beamform_dev(pbrt_ctx *ctx, const pbrt_apod_params *p, const void *d_data, const void *d_tx_delays, const void *d_elem,
                           const void *d_px, const void *d_pz, void *d_out) {
    BF_REQUEST(p);
    return beamform_dev(ctx, rq, d_data, d_elem, d_px, d_pz, d_out, d_tx_delays, nullptr);
}
int pbrt_apod_beamform_table_dev(pbrt_ctx *ctx, const pbrt_apod_params *p, const void *d_data, const void *d_table, const void *d_elem,
                                 const void *d_px, const void *d_pz, void *d_out) {
    BF_REQUEST(p);
    return beamform_dev(ctx, rq, d_data, d_elem, d_px, d_pz, d_out, nullptr, d_table);
}
int pbrt_capon_beamform(pbrt_ctx *ctx, const pbrt_capon_params *p, const float *iq, const float *tx_delays, const float *elem,
                        const float *px, const float *pz, float *out) {
    MAKE_REQUEST(ctx, CaponRequest, capon_request, p);
    return beamform_host(ctx, rq.bf, iq, tx_delays, elem, px, pz, out, &rq);
}
int pbrt_capon_beamform_dev(pbrt_ctx *ctx, const pbrt_capon_params *p, const void *d_iq, const void *d_tx_delays, const void *d_elem,
                            const void *d_px, const void *d_pz, void *d_out) {
    MAKE_REQUEST(ctx, CaponRequest, capon_request, p);
    return beamform_dev(ctx, rq.bf, d_iq, d_elem, d_px, d_pz, d_out, d_tx_delays, nullptr, &rq);
}
int pbrt_capon_beamform_table_dev(pbrt_ctx *ctx, const pbrt_capon_params *p, const void *d_iq, const void *d_table, const void *d_elem,
                                  const void *d_px, const void *d_pz, void *d_out) {
    MAKE_REQUEST(ctx, CaponRequest, capon_request, p);
    return beamform_dev(ctx, rq.bf, d_iq, d_elem, d_px, d_pz, d_out, nullptr, d_table, &rq);
}
int pbrt_coherence_beamform(pbrt_ctx *ctx, const pbrt_coherence_params *p, const float *iq, const float *tx_delays, const float *elem, const float *px, const float *pz, float *out) {
    MAKE_REQUEST(ctx, CoherenceRequest, coherence_request, p);
    return beamform_host(ctx, rq.bf, iq, tx_delays, elem, px, pz, out, nullptr, &rq);
}
int pbrt_coherence_beamform_dev(pbrt_ctx *ctx, const pbrt_coherence_params *p, const void *d_iq, const void *d_tx_delays, const void *d_elem, const void *d_px, const void *d_pz, void *d_out) {
    MAKE_REQUEST(ctx, CoherenceRequest, coherence_request, p);
    return beamform_dev(ctx, rq.bf, d_iq, d_elem, d_px, d_pz, d_out, d_tx_delays, nullptr, nullptr, &rq);
}
int pbrt_coherence_beamform_table_dev(pbrt_ctx *ctx, const pbrt_coherence_params *p, const void *d_iq, const void *d_table, const void *d_elem, const void *d_px, const void *d_pz, void *d_out) {
    MAKE_REQUEST(ctx, CoherenceRequest, coherence_request, p);
    return beamform_dev(ctx, rq.bf, d_iq, d_elem, d_px, d_pz, d_out, nullptr, d_table, nullptr, &rq);
}
int pbrt_scan_first_arrival_dev(pbrt_ctx *ctx, const pbrt_scan_params *p, const void *d_tx_delays, const void *d_elem, const void *d_px,
                                const void *d_pz, void *d_table) {
    BF_REQUEST(p);
    return first_arrival_dev(ctx, rq, d_tx_delays, d_elem, d_px, d_pz, d_table);
}
int pbrt_scan_convert_dev(pbrt_ctx *ctx, const pbrt_scan_convert_params *p, const void *d_src, const void *d_x, const void *d_z,
                          void *d_dst) {
    IMG_QUEUED(ctx, ScanConvertRequest, scan_convert_request, p, d_src, d_x, d_z, d_dst);
    return scan_convert_enqueue(ctx, rq, (const float *)d_src, (const float *)d_x, (const float *)d_z, (float *)d_dst);
}
int pbrt_scan_convert(pbrt_ctx *ctx, const pbrt_scan_convert_params *p, const float *src, const float *x, const float *z, float *dst) {
    IMG_STAGED(ctx, ScanConvertRequest, scan_convert_request, p, src, x, z, dst);
    auto [dsrc, dx, dz, ddst] = S.arrays(stage_in(src, rq.n_src), stage_in(x, p->nx), stage_in(z, p->nz), stage_out(dst, rq.n_dst));
    STAGED_RUN(S, scan_convert_enqueue(ctx, rq, dsrc, dx, dz, ddst));
}

int pbrt_iq_beamform_dev(pbrt_ctx *ctx, const pbrt_iq_params *p, const void *d_iq, const void *d_tx_delays, const void *d_elem,
                         const void *d_x, const void *d_z, void *d_out) {
    BF_REQUEST(p);
    return beamform_dev(ctx, rq, d_iq, d_elem, d_x, d_z, d_out, d_tx_delays, nullptr);
}
int pbrt_iq_beamform_table_dev(pbrt_ctx *ctx, const pbrt_iq_params *p, const void *d_iq, const void *d_table, const void *d_elem,
                               const void *d_x, const void *d_z, void *d_out) {
    BF_REQUEST(p);
    return beamform_dev(ctx, rq, d_iq, d_elem, d_x, d_z, d_out, nullptr, d_table);
}
int pbrt_iq_beamform(pbrt_ctx *ctx, const pbrt_iq_params *p, const float *iq, const float *tx_delays, const float *elem,
                     const float *x, const float *z, float *out) {
    BF_REQUEST(p);
    return beamform_host(ctx, rq, iq, tx_delays, elem, x, z, out);
}
int pbrt_rf2iq_dev(pbrt_ctx *ctx, uint32_t n_traces, uint32_t time_samples, float fs, float t0, float demod_freq,
                   uint32_t decimation, uint32_t K, const void *d_taps, const void *d_in, void *d_out) {
    IMG_QUEUED(ctx, Rf2iqRequest, rf2iq_request, n_traces, time_samples, fs, t0, demod_freq, decimation, K, d_taps, d_in, d_out);
    return rf2iq_enqueue(ctx, rq, (const float *)d_taps, (const float *)d_in, (float *)d_out);
}
int pbrt_rf2iq(pbrt_ctx *ctx, uint32_t n_traces, uint32_t time_samples, float fs, float t0, float demod_freq, uint32_t decimation,
               uint32_t K, const float *taps, const float *in, float *out) {
    IMG_STAGED(ctx, Rf2iqRequest, rf2iq_request, n_traces, time_samples, fs, t0, demod_freq, decimation, K, taps, in, out);
    auto [dh, din, dout] = S.arrays(stage_in(taps, 2 * (size_t)K + 1), stage_in(in, (size_t)n_traces * time_samples),
                                    stage_out(out, (size_t)n_traces * rq.Td * 2));
    STAGED_RUN(S, rf2iq_enqueue(ctx, rq, dh, din, dout));
}
int pbrt_iq_envelope_dev(pbrt_ctx *ctx, uint32_t n, const void *d_iq, void *d_env) {
    IMG_QUEUED(ctx, IqEnvRequest, iq_env_request, n, d_iq, d_env);
    return iq_env_enqueue(ctx, rq, (const float *)d_iq, (float *)d_env);
}
int pbrt_iq_envelope(pbrt_ctx *ctx, uint32_t n, const float *iq, float *env) {
    IMG_STAGED(ctx, IqEnvRequest, iq_env_request, n, iq, env);
    auto [din, dout] = S.arrays(stage_in(iq, 2 * (size_t)n), stage_out(env, n));
    STAGED_RUN(S, iq_env_enqueue(ctx, rq, din, dout));
}
#include "doppler_driver.h"  // pbrt_doppler_autocorr[_dev], pbrt_doppler_maps[_dev] (DESIGN D24): their launches and entry points

int pbrt_bf_beamform_dev(pbrt_ctx *ctx, const pbrt_bf_params *p, const void *d_data, const void *d_tx_delays, const void *d_elem,
                         const void *d_x, const void *d_z, void *d_out) {
    BF_REQUEST(p);
    return beamform_dev(ctx, rq, d_data, d_elem, d_x, d_z, d_out, d_tx_delays, nullptr);
}
int pbrt_bf_beamform_table_dev(pbrt_ctx *ctx, const pbrt_bf_params *p, const void *d_data, const void *d_table, const void *d_elem,
                               const void *d_x, const void *d_z, void *d_out) {
    BF_REQUEST(p);
    return beamform_dev(ctx, rq, d_data, d_elem, d_x, d_z, d_out, nullptr, d_table);
}
int pbrt_bf_beamform(pbrt_ctx *ctx, const pbrt_bf_params *p, const float *data, const float *tx_delays, const float *elem,
                     const float *x, const float *z, float *out) {
    BF_REQUEST(p);
    return beamform_host(ctx, rq, data, tx_delays, elem, x, z, out);
}
int pbrt_axial_fir_dev(pbrt_ctx *ctx, uint32_t nx, uint32_t nz, uint32_t K, const void *d_taps, const void *d_in, void *d_out) {
    IMG_QUEUED(ctx, FirRequest, fir_request, nx, nz, K, d_taps, d_in, d_out);
    return fir_enqueue(ctx, rq, (const float *)d_taps, (const float *)d_in, (float *)d_out);
}
int pbrt_axial_fir(pbrt_ctx *ctx, uint32_t nx, uint32_t nz, uint32_t K, const float *taps, const float *in, float *out) {
    IMG_STAGED(ctx, FirRequest, fir_request, nx, nz, K, taps, in, out);
    auto [dh, din, dout] = S.arrays(stage_in(taps, 2 * (size_t)K + 1), stage_in(in, (size_t)nx * nz), stage_out(out, (size_t)nx * nz));
    STAGED_RUN(S, fir_enqueue(ctx, rq, dh, din, dout));
}

int pbrt_das_beamform_dev(pbrt_ctx *ctx, const pbrt_das_params *p, const void *d_data, const void *d_tx_delays, const void *d_elem_x,
                          const void *d_x, const void *d_z, void *d_out) {
    BF_REQUEST(p, false);
    return beamform_dev(ctx, rq, d_data, d_elem_x, d_x, d_z, d_out, d_tx_delays, nullptr);
}
int pbrt_das_beamform_probe_dev(pbrt_ctx *ctx, const pbrt_das_params *p, const void *d_data, const void *d_tx_delays, const void *d_elem,
                                const void *d_x, const void *d_z, void *d_out) {
    BF_REQUEST(p, true);
    return beamform_dev(ctx, rq, d_data, d_elem, d_x, d_z, d_out, d_tx_delays, nullptr);
}
int pbrt_das_first_arrival_dev(pbrt_ctx *ctx, const pbrt_das_params *p, const void *d_tx_delays, const void *d_elem_x, const void *d_x,
                               const void *d_z, void *d_table) {
    BF_REQUEST(p, false);
    return first_arrival_dev(ctx, rq, d_tx_delays, d_elem_x, d_x, d_z, d_table);
}
int pbrt_das_first_arrival_probe_dev(pbrt_ctx *ctx, const pbrt_das_params *p, const void *d_tx_delays, const void *d_elem, const void *d_x,
                                     const void *d_z, void *d_table) {
    BF_REQUEST(p, true);
    return first_arrival_dev(ctx, rq, d_tx_delays, d_elem, d_x, d_z, d_table);
}
int pbrt_das_beamform_table_dev(pbrt_ctx *ctx, const pbrt_das_params *p, const void *d_data, const void *d_table, const void *d_elem_x,
                                const void *d_x, const void *d_z, void *d_out) {
    BF_REQUEST(p, false);
    return beamform_dev(ctx, rq, d_data, d_elem_x, d_x, d_z, d_out, nullptr, d_table);
}
int pbrt_das_beamform_table_probe_dev(pbrt_ctx *ctx, const pbrt_das_params *p, const void *d_data, const void *d_table, const void *d_elem,
                                      const void *d_x, const void *d_z, void *d_out) {
    BF_REQUEST(p, true);
    return beamform_dev(ctx, rq, d_data, d_elem, d_x, d_z, d_out, nullptr, d_table);
}
int pbrt_das_beamform(pbrt_ctx *ctx, const pbrt_das_params *p, const float *data, const float *tx_delays,
                      const float *elem_x, const float *x, const float *z, float *out) {
    BF_REQUEST(p, false);
    return beamform_host(ctx, rq, data, tx_delays, elem_x, x, z, out);
}
int pbrt_das_beamform_probe(pbrt_ctx *ctx, const pbrt_das_params *p, const float *data, const float *tx_delays,
                            const float *elem, const float *x, const float *z, float *out) {
    BF_REQUEST(p, true);
    return beamform_host(ctx, rq, data, tx_delays, elem, x, z, out);
}

int pbrt_envelope_dev(pbrt_ctx *ctx, uint32_t nx, uint32_t nz, const void *d_rf, void *d_env) {
    IMG_QUEUED(ctx, EnvRequest, env_request, IMG_FORM_DEV, nx, nz, d_rf, d_env, ctx->lds_limit, read_switches().env_general);
    return env_enqueue(ctx, rq, (const float *)d_rf, (float *)d_env);
}
int pbrt_envelope(pbrt_ctx *ctx, uint32_t nx, uint32_t nz, const float *rf, float *env) {
    IMG_STAGED(ctx, EnvRequest, env_request, IMG_FORM_HOST, nx, nz, rf, env, ctx->lds_limit, read_switches().env_general);
    auto [din, dout] = S.arrays(stage_in(rf, (size_t)nx * nz), stage_out(env, (size_t)nx * nz));
    STAGED_RUN(S, env_enqueue(ctx, rq, din, dout));
}
int pbrt_log_compress_dev(pbrt_ctx *ctx, uint32_t n, const void *d_env, float dynamic_range_db, void *d_out) {
    IMG_QUEUED(ctx, LogRequest, log_request, n, d_env, dynamic_range_db, d_out);
    return log_enqueue(ctx, rq, (const float *)d_env, (float *)d_out);
}
int pbrt_log_compress(pbrt_ctx *ctx, uint32_t n, const float *env, float dynamic_range_db, float *out) {
    IMG_STAGED(ctx, LogRequest, log_request, n, env, dynamic_range_db, out);
    auto [din, dout] = S.arrays(stage_in(env, n), stage_out(out, n));
    STAGED_RUN(S, log_enqueue(ctx, rq, din, dout));
}
int pbrt_us_apply_pulse_dev(pbrt_ctx *ctx, uint32_t n_traces, uint32_t time_samples, float fs, float frequency, float sigma,
                            const void *d_in, void *d_out) {
    IMG_QUEUED(ctx, PulseRequest, pulse_request, n_traces, time_samples, fs, frequency, sigma, d_in, d_out);
    return pulse_enqueue(ctx, rq, (const float *)d_in, (float *)d_out);
}
int pbrt_us_apply_pulse(pbrt_ctx *ctx, uint32_t n_traces, uint32_t time_samples, float fs, float frequency, float sigma,
                        const float *in, float *out) {
    IMG_STAGED(ctx, PulseRequest, pulse_request, n_traces, time_samples, fs, frequency, sigma, in, out);
    auto [din, dout] = S.arrays(stage_in(in, (size_t)n_traces * time_samples), stage_out(out, (size_t)n_traces * time_samples));
    STAGED_RUN(S, pulse_enqueue(ctx, rq, din, dout));
}

// ---- device buffers and the stream (ABI 5): what a caller needs to keep the us_render loop in HBM without another GPU library ----
int pbrt_ctx_synchronize(pbrt_ctx *c) {
    if (!c) return PBRT_E_INVALID;
    NOT_RECORDING(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ctx_settle(c);  // (a queued acquisition: its guard words are looked at now)
}

int pbrt_ctx_set_profiling(pbrt_ctx *c, int on) {
    if (!c) return PBRT_E_INVALID;
    c->profiling = on != 0;
    c->img_mask = 0;
    return PBRT_OK;
}

int pbrt_get_image_stats(pbrt_ctx *c, pbrt_image_stats *out) {
    if (!c || !out) return PBRT_E_INVALID;
    std::memset(out, 0, sizeof *out);
    NOT_RECORDING(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double *slot[IMG_STEPS] = {&out->pulse_ms, &out->das_ms, &out->envelope_ms, &out->log_ms};
    for (int i = 0; i < IMG_STEPS; ++i) {
        if (!(c->img_mask & (1u << i))) continue;
        float t = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&t, c->img_ev[2 * i], c->img_ev[2 * i + 1]));
        *slot[i] = t;
    }
    out->das_model_bytes = c->img_das_bytes;
    out->measured = c->img_mask;
    return PBRT_OK;
}

int pbrt_dev_alloc(pbrt_ctx *c, uint64_t bytes, void **out) {
    if (!c || !out) return PBRT_E_INVALID;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, (size_t)std::max<uint64_t>(bytes, 16));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return c->fail(PBRT_E_NOMEM, "pbrt_dev_alloc(%llu): %s", (unsigned long long)bytes, hipGetErrorString(e));
    }
    *out = p;
    return PBRT_OK;
}

int pbrt_dev_free(pbrt_ctx *c, void *p) {
    if (!c) return PBRT_E_INVALID;
    if (!p) return PBRT_OK;
    NOT_RECORDING(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // queued work may still read or write it
    (void)ctx_settle(c);
    c->work.invalidate_recordings();  // (a recording may hold this pointer)
    HIPCHK(c, hipFree(p));
    return PBRT_OK;
}

int pbrt_dev_upload(pbrt_ctx *c, void *dst_dev, const void *src_host, uint64_t bytes) {
    if (!c) return PBRT_E_INVALID;
    NEED(c, (dst_dev && src_host) || bytes == 0);
    if (!bytes) return PBRT_OK;
    NOT_RECORDING(c);
    HIPCHK(c, hipSetDevice(c->device));
    // in stream order behind the queued kernels; a pageable source is staged before the call returns, so the caller may reuse it
    HIPCHK(c, hipMemcpyAsync(dst_dev, src_host, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    return PBRT_OK;
}

int pbrt_dev_download(pbrt_ctx *c, void *dst_host, const void *src_dev, uint64_t bytes) {
    if (!c) return PBRT_E_INVALID;
    NEED(c, (dst_host && src_dev) || bytes == 0);
    NOT_RECORDING(c);
    HIPCHK(c, hipSetDevice(c->device));
    if (bytes) HIPCHK(c, hipMemcpyAsync(dst_host, src_dev, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ctx_settle(c);  // an acquisition queued ahead of this copy that tripped its guard makes the copy's content invalid
}

// ---- the queued chain as one submission (include/pbrt_hip.h) ------------------------------------------------------------------
struct pbrt_graph {
    pbrt_ctx *ctx = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    pbrt_ctx::PendingAcq pend;  // what the recorded acquisition leaves for us_finish (inactive: the recording holds none)
    uint64_t epoch = 0;         // ctx->work.epoch() at the end of the recording
    uint64_t das_bytes = 0;
    uint64_t rows_gen = 0;      // the counter rows the recorded acquisition expects clean (it was recorded without their fill command)
    size_t rows_bytes = 0;
};

int pbrt_ctx_record_begin(pbrt_ctx *c) {
    if (!c) return PBRT_E_INVALID;
    if (int rc = ctx_settle(c)) return rc;  // (also: no recording inside a recording)
    HIPCHK(c, hipSetDevice(c->device));
    // relaxed: the recorded entry points query function attributes and free memory, calls a stricter mode refuses on any thread
    HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
    c->recording = true;
    c->rec_failed = false;
    c->rec_msg.clear();
    return PBRT_OK;
}

int pbrt_ctx_record_end(pbrt_ctx *c, pbrt_graph **out) {
    if (!c || !out) return PBRT_E_INVALID;
    *out = nullptr;
    if (!c->recording) return c->fail(PBRT_E_INVALID, "pbrt_ctx_record_end without pbrt_ctx_record_begin");
    c->recording = false;
    pbrt_ctx::PendingAcq P = c->pend;
    c->pend.active = false;  // (nothing ran)
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(c->stream, &g);
    if (e != hipSuccess || !g) {
        (void)hipGetLastError();
        return c->fail(PBRT_E_DEVICE, "hipStreamEndCapture: %s (a call inside the recording failed or waited)", hipGetErrorString(e));
    }
    if (c->rec_failed) {  // (the capture itself is intact, but what it holds is not the chain the caller meant)
        (void)hipGraphDestroy(g);
        return c->fail(PBRT_E_INVALID, "a call inside the recording failed: %s", c->rec_msg.c_str());
    }
    hipGraphExec_t x = nullptr;
    e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipGraphDestroy(g);
        return c->fail(PBRT_E_DEVICE, "hipGraphInstantiate: %s", hipGetErrorString(e));
    }
    pbrt_graph *G = new pbrt_graph;
    G->ctx = c;
    G->graph = g;
    G->exec = x;
    G->pend = P;
    G->pend.timed = false;
    G->epoch = c->work.epoch();
    G->das_bytes = c->img_das_bytes;
    if (P.active) {
        G->rows_gen = c->us_rows_gen;
        G->rows_bytes = c->us_rows_bytes;
    }
    *out = G;
    return PBRT_OK;
}

int pbrt_graph_launch(pbrt_graph *G) {
    if (!G) return PBRT_E_INVALID;
    pbrt_ctx *c = G->ctx;
    if (int rc = ctx_settle(c)) return rc;
    if (G->epoch != c->work.epoch())
        return c->fail(PBRT_E_INVALID, "the recording is stale: memory or tables it refers to were freed or replaced since it was made; record again");
    if (G->pend.active && (c->us_rows_gen != G->rows_gen || c->us_rows_bytes != G->rows_bytes))
        return c->fail(PBRT_E_INVALID, "the recording is stale: another acquisition (or one that failed) used the counters since it was made; record again");
    HIPCHK(c, hipSetDevice(c->device));
    ++c->call_seq;
    c->work.touch_all(c->call_seq);
    HIPCHK(c, hipGraphLaunch(G->exec, c->stream));
    c->pend = G->pend;
    c->img_das_bytes = G->das_bytes;
    return PBRT_OK;
}

int pbrt_graph_destroy(pbrt_graph *G) {
    if (!G) return PBRT_OK;
    pbrt_ctx *c = G->ctx;
    (void)hipSetDevice(c->device);
    if (!c->recording) (void)hipStreamSynchronize(c->stream);  // a replay may still run
    if (G->exec) (void)hipGraphExecDestroy(G->exec);
    if (G->graph) (void)hipGraphDestroy(G->graph);
    delete G;
    return PBRT_OK;
}

}  // extern "C"
