// The pure predicates the argument checks of the api_*.cpp files share.  Host arithmetic only, no HIP: compiles with a plain C++ compiler
// (tests/api_checks_check.cpp walks them).  They answer yes or no; the refusal's code and text stay at the caller's fail(...).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace pt {

// do [a, a + na) and [b, b + nb) share a byte?  A null pointer or an empty range overlaps nothing (no caller passes an empty one: every
// length is that of a frame the checks before have found non-empty, or a constant)
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && na && nb && pa < pb + nb && pb < pa + na;
}
// `align`: a power of two.  A null pointer is aligned
inline bool misaligned(const void* p, size_t align) { return ((uintptr_t)p & (uintptr_t)(align - 1)) != 0; }
inline bool all_finite_positive(std::initializer_list<float> values) {
    for (float v : values)
        if (!(std::isfinite(v) && v > 0.0f)) return false;
    return true;
}
// the frame bounds of the stages that index pixels with 32 bits: width and height up to 2^24 ...
inline bool frame_side_too_large(uint32_t width, uint32_t height) { return width > (1u << 24) || height > (1u << 24); }
// ... and fewer than 2^32 pixels.  An empty frame is not too large: the callers refuse it with a message of its own
inline bool frame_too_large(uint32_t width, uint32_t height) { return frame_side_too_large(width, height) || (((uint64_t)width * height) >> 32) != 0; }
// what is wrong with a caller's scratch buffer of `have` bytes where `need` are asked for: the first that applies, in this order
enum class Scratch { OK, MISSING, TOO_SMALL, MISALIGNED };
inline Scratch scratch_verdict(const void* p, size_t have, size_t need, size_t align) {
    return !p ? Scratch::MISSING : have < need ? Scratch::TOO_SMALL : misaligned(p, align) ? Scratch::MISALIGNED : Scratch::OK;
}
// is one of the call's n_outs output pointers (null ones among them, which are none) one of the three inputs a, b, c?
inline bool output_is_one_of(const void* const* outs, int n_outs, const void* a, const void* b, const void* c) {
    for (int i = 0; i < n_outs; ++i)
        if (outs[i] && (outs[i] == a || outs[i] == b || outs[i] == c)) return true;
    return false;
}
// what is wrong with the id buffers and the table of a motion-aware accumulation (include/mi355pt_motion.h): the first that applies, in
// this order.  ids_prev may be null; `outs`: the call's n_outs output pointers (null ones among them) and, for the rectified form, its scratch
enum class Motion { OK, MISSING, NO_ENTRIES, MISALIGNED, ALIASES_OUTPUT };
inline Motion motion_verdict(const void* ids_cur, const void* ids_prev, const void* table, uint32_t n_entries, size_t table_align, const void* const* outs,
                             int n_outs) {
    if (!ids_cur || !table) return Motion::MISSING;
    if (n_entries == 0u) return Motion::NO_ENTRIES;
    if (misaligned(table, table_align)) return Motion::MISALIGNED;
    return output_is_one_of(outs, n_outs, ids_cur, ids_prev, table) ? Motion::ALIASES_OUTPUT : Motion::OK;
}

}  // namespace pt
