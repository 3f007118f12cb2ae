// TEST INFRASTRUCTURE ONLY.  csrc/budget_plan.hpp on its own: a plain C++ program (no HIP), built by tests/test_budget.py with g++ and a
// second time with -fsanitize=address,undefined.
//   budget_plan_check <seed> <n>          the fixed corners, then n seeded cases of the formula against its definition by search; prints
//                                         "ok <cases>" and exits 0, or the first failing line and 1
//   budget_plan_check spp <lmin bits> <base> <max> <target bits>     prints budget_spp(...) — the Python tests feed it the corners
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

#include "budget_plan.hpp"

using namespace pt;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// the definition, by search over j with an exact power of two (ldexp of a float by j is exact short of overflow)
static uint32_t by_definition(float lmin, uint32_t base, uint32_t max, float target) {
    const float a = lmin + 1.0f;
    for (int j = 0; j < 32; ++j) {
        const uint64_t n = (uint64_t)base << j;
        if (std::ldexp(a, j) >= target || n == max) return (uint32_t)n;
    }
    return 0u;
}

int main(int argc, char** argv) {
    if (argc == 6 && std::strcmp(argv[1], "spp") == 0) {
        std::printf("%u\n", budget_spp(from_bits((uint32_t)std::strtoul(argv[2], nullptr, 0)), (uint32_t)std::strtoul(argv[3], nullptr, 0),
                                       (uint32_t)std::strtoul(argv[4], nullptr, 0), from_bits((uint32_t)std::strtoul(argv[5], nullptr, 0))));
        return 0;
    }
    if (argc != 3) { std::fprintf(stderr, "usage: %s <seed> <n> | spp <lmin bits> <base> <max> <target bits>\n", argv[0]); return 2; }
    const unsigned seed = (unsigned)std::strtoul(argv[1], nullptr, 0);
    const long n = std::strtol(argv[2], nullptr, 0);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();

    // the parameters' verdicts, in their order
    CHECK(budget_params_verdict(4, 32, 8.0f) == BudgetParams::OK);
    CHECK(budget_params_verdict(2, 2, 1.0f) == BudgetParams::OK);
    CHECK(budget_params_verdict(0, 0, 0.0f) == BudgetParams::BASE);          // a zeroed struct is refused, base first
    CHECK(budget_params_verdict(1, 32, 8.0f) == BudgetParams::BASE);
    CHECK(budget_params_verdict(6, 32, 8.0f) == BudgetParams::BASE);
    CHECK(budget_params_verdict(4, 2, 8.0f) == BudgetParams::MAX);
    CHECK(budget_params_verdict(4, 24, 8.0f) == BudgetParams::MAX);
    CHECK(budget_params_verdict(4, 0x80000000u, 8.0f) == BudgetParams::OK);
    CHECK(budget_params_verdict(4, 32, 0.5f) == BudgetParams::TARGET);
    CHECK(budget_params_verdict(4, 32, inf) == BudgetParams::TARGET);
    CHECK(budget_params_verdict(4, 32, nan) == BudgetParams::TARGET);
    CHECK(budget_params_verdict(4, 2, nan) == BudgetParams::MAX);            // the first that applies

    // the carry's verdict
    int a = 0, b = 0, c = 0, d = 0;
    CHECK(budget_carry_verdict(nullptr, nullptr, nullptr, 0, nullptr) == BudgetCarry::STATIC);
    CHECK(budget_carry_verdict(&a, &b, &c, 3, nullptr) == BudgetCarry::TABLE);
    CHECK(budget_carry_verdict(nullptr, nullptr, &c, 0, nullptr) == BudgetCarry::TABLE);      // (then motion_verdict refuses it)
    CHECK(budget_carry_verdict(&a, &b, nullptr, 0, &d) == BudgetCarry::FLOW);
    CHECK(budget_carry_verdict(nullptr, nullptr, nullptr, 0, &d) == BudgetCarry::FLOW);
    CHECK(budget_carry_verdict(&a, &b, &c, 3, &d) == BudgetCarry::BOTH);
    CHECK(budget_carry_verdict(&a, nullptr, nullptr, 0, nullptr) == BudgetCarry::IDS_ALONE);
    CHECK(budget_carry_verdict(nullptr, &b, nullptr, 0, nullptr) == BudgetCarry::IDS_ALONE);
    CHECK(budget_carry_verdict(nullptr, nullptr, nullptr, 2, nullptr) == BudgetCarry::IDS_ALONE);

    // the formula at its corners
    CHECK(budget_spp(0.0f, 4, 32, 8.0f) == 32);                               // no history: 1 * 2^3 >= 8
    CHECK(budget_spp(0.0f, 4, 16, 8.0f) == 16);                               // ... capped
    CHECK(budget_spp(7.0f, 4, 32, 8.0f) == 4);                                // Lmin + 1 at the target
    CHECK(budget_spp(std::nextafter(7.0f, 0.0f), 4, 32, 8.0f) == 8);          // one ulp below: 8 - ulp is a binary32 number
    CHECK(budget_spp(std::nextafter(1.0f, 0.0f), 4, 32, 2.0f) == 4);          // (1 - 2^-24) + 1 rounds to 2: rounded ONCE, then compared
    CHECK(budget_spp(6.5f, 4, 32, 8.0f) == 8);                                // just below
    CHECK(budget_spp(7.5f, 4, 32, 8.0f) == 4);                                // above
    CHECK(budget_spp(3.0f, 4, 32, 8.0f) == 8);                                // 4 * 2 >= 8
    CHECK(budget_spp(2.9f, 4, 32, 8.0f) == 16);
    CHECK(budget_spp(0.0f, 4, 32, 1.0f) == 4 && budget_spp(31.0f, 4, 32, 1.0f) == 4);      // target 1: every tile at base
    CHECK(budget_spp(0.0f, 8, 8, 32.0f) == 8);                                // base == max
    CHECK(budget_spp(0.0f, 4, 64, 5.0f) == 32);                               // a target that is no power of two: 2^3 >= 5
    CHECK(budget_spp(1.5f, 4, 64, 5.0f) == 8 && budget_spp(1.4f, 4, 64, 5.0f) == 16);
    CHECK(budget_spp(inf, 4, 32, 8.0f) == 4);
    CHECK(budget_spp(0.0f, 2, 0x80000000u, 3.0e38f) == 0x80000000u);          // every doubling, no overflow of the count
    CHECK(budget_spp(3.0e38f, 2, 0x80000000u, 3.4e38f) == 4);                 // the reach overflows to +inf and ends the loop

    // clamp, rendered count, credit
    CHECK(budget_clamp(0, 4, 32) == 4 && budget_clamp(3, 4, 32) == 4 && budget_clamp(4, 4, 32) == 4 && budget_clamp(33, 4, 32) == 32 &&
          budget_clamp(0xffffffffu, 4, 32) == 32 && budget_clamp(12, 4, 32) == 12);
    CHECK(budget_rendered(0, 4, 32) == 4 && budget_rendered(8, 4, 32) == 8 && budget_rendered(12, 4, 32) == 16 && budget_rendered(1000, 4, 32) == 32 &&
          budget_rendered(0xffffffffu, 2, 0x80000000u) == 0x80000000u);
    CHECK(!budget_has_credit(4, 4) && !budget_has_credit(2, 4) && budget_has_credit(8, 4));
    CHECK(budget_credit(8, 4) == 1.0f && budget_credit(32, 4) == 7.0f && budget_credit(12, 4) == 2.0f);

    // seeded cases against the definition
    std::mt19937 rng(seed);
    long cases = 0;
    for (long i = 0; i < n; ++i, ++cases) {
        const uint32_t lb = 1u + rng() % 5u, base = 1u << lb, max = 1u << (lb + rng() % (32u - lb));
        float target = 1.0f + (float)(rng() % 4096u) / 64.0f;
        if (rng() % 8u == 0u) target = std::ldexp(1.0f, (int)(rng() % 12u));
        float lmin = (float)(rng() % 8192u) / 128.0f;
        if (rng() % 8u == 0u) lmin = 0.0f;
        if (rng() % 16u == 0u) lmin = std::nextafter(target - 1.0f, (rng() & 1u) ? 0.0f : inf);
        if (lmin < 0.0f) lmin = 0.0f;
        const uint32_t got = budget_spp(lmin, base, max, target), want = by_definition(lmin, base, max, target);
        if (got != want) {
            std::printf("FAILED case %ld: lmin %a base %u max %u target %a: %u, definition %u\n", i, lmin, base, max, target, got, want);
            ++failures;
            break;
        }
        CHECK(budget_pow2(got) && got >= base && got <= max);
    }
    if (failures) return 1;
    std::printf("ok %ld\n", cases);
    return 0;
}
