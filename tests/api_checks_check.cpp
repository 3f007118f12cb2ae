// The pure argument predicates of csrc/api_checks.hpp (host only), which the *_check functions of the api_*.cpp files share.  Walks
//   overlap          over every placement of two ranges of 0 .. 4 bytes in a window of 12, and with either or both pointers null, against
//                    the definition "some byte lies in both";
//   misaligned       over the addresses 0 .. 63 for the alignments 4 and 16;
//   all_finite_positive  on 0, -0, the smallest denormal, NaN, +-inf and 1, alone and in lists;
//   frame_side_too_large / frame_too_large  at 2^24 and 2^24 + 1 on either side, at 65536 x 65535, 65536 x 65536, 2^24 x 256 and at 0;
//   scratch_verdict  in its four outcomes and their precedence: missing, then too small, then misaligned.
// tests/test_api_checks.py.
//   usage: api_checks_check
//   prints one line "ok cases"; exits 1 with a message at the first violation
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "api_checks.hpp"

using namespace pt;

static long cases = 0;
static void fail(const char* what, long a, long b, long c, long d) {
    std::printf("FAIL %s (%ld, %ld, %ld, %ld)\n", what, a, b, c, d);
    std::exit(1);
}
#define CHECK4(c, x, y, z, w) do { ++cases; if (!(c)) fail(#c, (long)(x), (long)(y), (long)(z), (long)(w)); } while (0)
#define CHECK(c) CHECK4(c, 0, 0, 0, 0)

int main() {
    // overlap: [ao, ao + na) and [bo, bo + nb) inside a window of 12 bytes
    const int WINDOW = 12, MAXLEN = 4;
    alignas(16) static unsigned char window[WINDOW + 4];
    for (int na = 0; na <= MAXLEN; ++na)
        for (int ao = 0; ao + na <= WINDOW; ++ao)
            for (int nb = 0; nb <= MAXLEN; ++nb)
                for (int bo = 0; bo + nb <= WINDOW; ++bo) {
                    bool shared = false;
                    for (int i = 0; i < WINDOW; ++i) shared = shared || (i >= ao && i < ao + na && i >= bo && i < bo + nb);
                    CHECK4(overlap(window + ao, (size_t)na, window + bo, (size_t)nb) == shared, ao, na, bo, nb);
                }
    for (int n = 0; n <= MAXLEN; ++n)
        for (int m = 0; m <= MAXLEN; ++m) {
            for (int o = 0; o + m <= WINDOW; ++o) {
                CHECK4(!overlap(nullptr, (size_t)n, window + o, (size_t)m), n, o, m, 0);
                CHECK4(!overlap(window + o, (size_t)m, nullptr, (size_t)n), o, m, n, 0);
            }
            CHECK4(!overlap(nullptr, (size_t)n, nullptr, (size_t)m), n, m, 0, 0);
        }

    // misaligned: a null pointer is aligned
    for (size_t align : {(size_t)4, (size_t)16})
        for (uintptr_t a = 0; a < 64; ++a) CHECK4(misaligned((const void*)a, align) == (a % align != 0), a, align, 0, 0);

    // all_finite_positive
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), tiny = std::numeric_limits<float>::denorm_min();
    CHECK(!all_finite_positive({0.0f}));
    CHECK(!all_finite_positive({-0.0f}));
    CHECK(all_finite_positive({tiny}));
    CHECK(!all_finite_positive({nan}));
    CHECK(!all_finite_positive({inf}));
    CHECK(!all_finite_positive({-inf}));
    CHECK(all_finite_positive({1.0f}));
    CHECK(all_finite_positive({1.0f, tiny, 1.0f}));
    CHECK(!all_finite_positive({1.0f, nan}));
    CHECK(!all_finite_positive({0.0f, 1.0f}));
    CHECK(!all_finite_positive({1.0f, 1.0f, inf}));

    // the frame bounds: sides up to 2^24, fewer than 2^32 pixels; an empty frame is not too large
    const uint32_t S = 1u << 24;
    CHECK(!frame_side_too_large(S, 1u) && !frame_side_too_large(1u, S) && !frame_side_too_large(S, S));
    CHECK(frame_side_too_large(S + 1u, 1u));
    CHECK(frame_side_too_large(1u, S + 1u));
    CHECK(!frame_side_too_large(0u, 0u));
    CHECK(!frame_too_large(S, 1u) && !frame_too_large(1u, S));
    CHECK(frame_too_large(S + 1u, 1u));
    CHECK(frame_too_large(1u, S + 1u));
    CHECK(!frame_too_large(65536u, 65535u) && !frame_too_large(65535u, 65536u));
    CHECK(frame_too_large(65536u, 65536u));
    CHECK(!frame_too_large(S, 255u));
    CHECK(frame_too_large(S, 256u) && !frame_side_too_large(S, 256u));
    CHECK(!frame_too_large(0u, 0u) && !frame_too_large(0u, S) && !frame_too_large(S, 0u));

    // scratch_verdict: missing, then too small, then misaligned
    const void* p = window;          // 16-byte aligned
    const void* q = window + 4;      // 4-byte aligned only
    CHECK(scratch_verdict(p, 64, 64, 16) == Scratch::OK);
    CHECK(scratch_verdict(p, 0, 0, 16) == Scratch::OK);
    CHECK(scratch_verdict(q, 64, 64, 4) == Scratch::OK);
    CHECK(scratch_verdict(nullptr, 64, 64, 16) == Scratch::MISSING);
    CHECK(scratch_verdict(p, 63, 64, 16) == Scratch::TOO_SMALL);
    CHECK(scratch_verdict(q, 64, 64, 16) == Scratch::MISALIGNED);
    CHECK(scratch_verdict(nullptr, 0, 64, 16) == Scratch::MISSING);       // missing before too small
    CHECK(scratch_verdict(q, 63, 64, 16) == Scratch::TOO_SMALL);          // too small before misaligned
    CHECK(scratch_verdict(window + 1, 64, 64, 4) == Scratch::MISALIGNED);

    std::printf("ok %ld\n", cases);
    return 0;
}
