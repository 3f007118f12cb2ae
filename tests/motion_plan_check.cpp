// TEST INFRASTRUCTURE ONLY.  csrc/motion_plan.hpp on its own (plain g++, no HIP): seeded instance motions — translation, rotation about a
// random axis, non-uniform scale, all three — between two camera positions, and for each
//   - record 0 and the record of a bytewise unmoved instance are EXACTLY a = n = I, b = c_cur - c_prev (the double difference rounded once);
//   - a random local point placed by l2w_cur, taken to the current render space, carried through the record (in long double) lands where
//     l2w_prev places the same local point in the previous render space, within a bound from the f32 rounding of the record's entries:
//     (|a| |X| + |b|) 2^-24 per component, plus the double arithmetic's own error, 1e-11 absolute;
//   - n^T a = I within the same kind of bound (n is the inverse transpose of a);
// then the refusals: n == 0, a NaN entry, an infinite entry, a singular linear part (a zero row, two equal columns), in the current and in
// the previous set and for an instance that did not move; the output is untouched by a refused call.
// usage: motion_plan_check <seed> <n_instances>   ->   "ok <records>"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "motion_plan.hpp"

using namespace pt;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

namespace {

std::mt19937 rng;
double uni(double a, double b) { return a + (b - a) * (double)(rng() >> 8) * (1.0 / 16777216.0); }

// T(t) R(axis, angle) S(s) as a column-major 4x4 of floats
void trs(const double t[3], const double axis[3], double angle, const double s[3], float out[16]) {
    const double l = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    const double x = axis[0] / l, y = axis[1] / l, z = axis[2] / l, c = std::cos(angle), sn = std::sin(angle), k = 1.0 - c;
    const double r[3][3] = {{c + x * x * k, x * y * k - z * sn, x * z * k + y * sn},
                            {y * x * k + z * sn, c + y * y * k, y * z * k - x * sn},
                            {z * x * k - y * sn, z * y * k + x * sn, c + z * z * k}};
    for (int col = 0; col < 3; ++col) {
        for (int row = 0; row < 3; ++row) out[4 * col + row] = (float)(r[row][col] * s[col]);
        out[4 * col + 3] = 0.0f;
    }
    for (int row = 0; row < 3; ++row) out[12 + row] = (float)t[row];
    out[15] = 1.0f;
}
void place(const float m[16], const double p[3], long double o[3]) {
    for (int r = 0; r < 3; ++r) o[r] = (long double)m[r] * p[0] + (long double)m[4 + r] * p[1] + (long double)m[8 + r] * p[2] + (long double)m[12 + r];
}
bool is_static(const MotionXform& e, const float cc[3], const float cp[3]) {
    for (int k = 0; k < 9; ++k) {
        const float want = (k % 4 == 0) ? 1.0f : 0.0f;
        if (std::memcmp(&e.a[k], &want, 4) != 0 || std::memcmp(&e.n[k], &want, 4) != 0) return false;
    }
    for (int i = 0; i < 3; ++i) {
        const float want = (float)((double)cc[i] - (double)cp[i]), zero = 0.0f;
        if (std::memcmp(&e.b[i], &want, 4) != 0 || std::memcmp(&e.pad[i], &zero, 4) != 0) return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: motion_plan_check <seed> <n_instances>\n"); return 2; }
    rng.seed((unsigned)std::atoi(argv[1]));
    const uint32_t n = (uint32_t)std::atoi(argv[2]);
    static_assert(sizeof(MotionXform) == 96, "six float4");
    float cc[3], cp[3];
    for (int i = 0; i < 3; ++i) { cc[i] = (float)uni(-5.0, 5.0); cp[i] = (float)uni(-5.0, 5.0); }
    if (n == 0) {      // refused, and the output stays
        MotionXform out; std::memset(&out, 0x5a, sizeof(out));
        MotionXform keep = out;
        const float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        CHECK(!motion_table(cc, cp, m, m, 0, &out));
        CHECK(std::memcmp(&out, &keep, sizeof(out)) == 0);
        std::printf("ok 0\n");
        return 0;
    }
    std::vector<float> cur(16 * (size_t)n), prev(16 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        const int kind = (int)(i % 5u);      // 0 unmoved, 1 translation, 2 rotation, 3 non-uniform scale, 4 all three
        double t[3], ax[3], s[3] = {1.0, 1.0, 1.0};
        for (int k = 0; k < 3; ++k) { t[k] = uni(-3.0, 3.0); ax[k] = uni(-1.0, 1.0) + (k == 1 ? 1.5 : 0.0); }
        const double ang = uni(-3.0, 3.0);
        if (i & 1u) for (int k = 0; k < 3; ++k) s[k] = uni(0.5, 2.0);
        trs(t, ax, ang, s, &prev[16 * (size_t)i]);
        double t2[3] = {t[0], t[1], t[2]}, s2[3] = {s[0], s[1], s[2]};
        double ang2 = ang;
        if (kind == 1 || kind == 4) for (int k = 0; k < 3; ++k) t2[k] += uni(-0.5, 0.5);
        if (kind == 2 || kind == 4) ang2 += uni(-0.3, 0.3);
        if (kind == 3 || kind == 4) for (int k = 0; k < 3; ++k) s2[k] *= uni(0.8, 1.25);
        trs(t2, ax, ang2, s2, &cur[16 * (size_t)i]);
        if (kind == 0) std::memcpy(&cur[16 * (size_t)i], &prev[16 * (size_t)i], 16 * sizeof(float));
    }
    std::vector<MotionXform> out((size_t)n + 1);
    CHECK(motion_table(cc, cp, cur.data(), prev.data(), n, out.data()));
    CHECK(is_static(out[0], cc, cp));
    const long double u = 5.9604644775390625e-8L;      // 2^-24
    for (uint32_t i = 0; i < n; ++i) {
        const MotionXform& e = out[(size_t)i + 1];
        if (i % 5u == 0u) { CHECK(is_static(e, cc, cp)); continue; }
        for (int k = 0; k < 3; ++k) CHECK(e.pad[k] == 0.0f);
        for (int trial = 0; trial < 8; ++trial) {
            const double p[3] = {uni(-2.0, 2.0), uni(-2.0, 2.0), uni(-2.0, 2.0)};
            long double wc[3], wp[3];
            place(&cur[16 * (size_t)i], p, wc);
            place(&prev[16 * (size_t)i], p, wp);
            for (int r = 0; r < 3; ++r) {
                long double got = e.b[r], mag = std::fabs((long double)e.b[r]);
                for (int c = 0; c < 3; ++c) {
                    const long double x = wc[c] - (long double)cc[c];
                    got += (long double)e.a[3 * r + c] * x;
                    mag += std::fabs((long double)e.a[3 * r + c] * x);
                }
                const long double want = wp[r] - (long double)cp[r];
                // each of the four entries is within 2^-24 relative of its double value; the double arithmetic behind them (an inverse of
                // a matrix of condition <= 16 here, two products, entries and coordinates below 20) is off by less than 1e-11 ABSOLUTE —
                // absolute, because an entry that is 0 in exact arithmetic comes out as 1e-16, not as 0
                CHECK(std::fabs(got - want) <= mag * u + 1e-11L);
            }
        }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                long double s = 0.0L, mag = 0.0L;
                for (int k = 0; k < 3; ++k) { s += (long double)e.n[3 * k + r] * e.a[3 * k + c]; mag += std::fabs((long double)e.n[3 * k + r] * e.a[3 * k + c]); }
                CHECK(std::fabs(s - (r == c ? 1.0L : 0.0L)) <= mag * 2.0L * u + 1e-11L);
            }
    }
    // refusals: the output keeps its bytes
    std::vector<MotionXform> keep = out;
    const size_t last = 16 * (size_t)(n - 1);
    for (int which = 0; which < 2; ++which) {
        std::vector<float>& set = which == 0 ? cur : prev;
        const std::vector<float> saved = set;
        set[last + 5] = NAN;
        CHECK(!motion_table(cc, cp, cur.data(), prev.data(), n, out.data()));
        set = saved; set[last + 13] = INFINITY;
        CHECK(!motion_table(cc, cp, cur.data(), prev.data(), n, out.data()));
        set = saved; set[last + 0] = set[last + 4] = set[last + 8] = 0.0f;           // a zero row
        CHECK(!motion_table(cc, cp, cur.data(), prev.data(), n, out.data()));
        set = saved; for (int r = 0; r < 3; ++r) set[last + 4 + r] = set[last + r];    // two equal columns
        CHECK(!motion_table(cc, cp, cur.data(), prev.data(), n, out.data()));
        set = saved;
    }
    {   // singular AND unmoved: refused all the same
        const std::vector<float> sc = cur, sp = prev;
        for (int k = 0; k < 12; ++k) cur[k] = prev[k] = 0.0f;
        CHECK(!motion_table(cc, cp, cur.data(), prev.data(), n, out.data()));
        cur = sc; prev = sp;
    }
    CHECK(std::memcmp(out.data(), keep.data(), out.size() * sizeof(MotionXform)) == 0);
    CHECK(motion_table(cc, cp, cur.data(), prev.data(), n, out.data()));
    CHECK(std::memcmp(out.data(), keep.data(), out.size() * sizeof(MotionXform)) == 0);      // the same table again
    std::printf("ok %u\n", n + 1u);
    return 0;
}
