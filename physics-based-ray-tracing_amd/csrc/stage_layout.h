// The staging area of a call that takes host arrays (pbrt_api.hip Stage: the leaf operators, the host forms of the image steps and of
// the beamformers, pbrt_integrator_sample).  The caller names each array once -- where it comes from or goes to, its element type, its
// length -- and the layout follows from that list: every array on a 16-byte boundary, the total what the workspace is asked for.  No
// caller writes a byte count, so no array lies beyond the allocation.  Plain host code (tests/native/stage_layout_check.cpp builds it).
#pragma once
#include <array>
#include <cstddef>

// one array of a staged call, n elements of T.  input: src is uploaded, and a null src keeps its slot and gives a null device
// pointer; dst, when there is one, is downloaded as the call finishes
template <class T>
struct StageArray {
    const T *src;
    T *dst;
    size_t n;
    bool input;
    size_t bytes() const { return n * sizeof(T); }
};
template <class T> static inline StageArray<T> stage_in(const T *h, size_t n) { return {h, nullptr, n, true}; }
template <class T> static inline StageArray<T> stage_out(T *h, size_t n) { return {nullptr, h, n, false}; }
template <class T> static inline StageArray<T> stage_inout(T *h, size_t n) { return {h, h, n, true}; }

static inline size_t stage_slot(size_t bytes) { return (bytes + 15) & ~size_t(15); }
template <size_t N> struct StageLayout { std::array<size_t, N> offset; size_t total; };
// a function of the byte lengths alone, in the order of the list
template <size_t N>
static inline StageLayout<N> stage_layout(const std::array<size_t, N> &bytes) {
    StageLayout<N> L{};
    for (size_t i = 0; i < N; ++i) {
        L.offset[i] = L.total;
        L.total += stage_slot(bytes[i]);
    }
    return L;
}
template <class... T>
static inline StageLayout<sizeof...(T)> stage_layout(const StageArray<T> &...a) { return stage_layout<sizeof...(T)>({{a.bytes()...}}); }
