// The pure part of the sample budget (include/mi355pt_budget.h): the predicates of api_budget.cpp's argument checks and the budget formula,
// which the probe kernel (pt_kernels_budget.hip) and the host share as one text.  Host arithmetic only, no HIP header: compiles with a
// plain C++ compiler (tests/budget_plan_check.cpp walks it, plain and under ASan + UBSan).  The predicates answer with a verdict; the
// refusal's code and text stay at the caller's fail(...).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "api_checks.hpp"
#include "flow_checks.hpp"

#if defined(__HIPCC__)
#define PT_BUDGET_HD __host__ __device__
#else
#define PT_BUDGET_HD
#endif

namespace pt {

inline bool budget_pow2(uint32_t v) { return v != 0u && (v & (v - 1u)) == 0u; }

// what is wrong with a mi355pt_budget_params: the first that applies, in this order
enum class BudgetParams { OK, BASE, MAX, TARGET };
inline BudgetParams budget_params_verdict(uint32_t base_spp, uint32_t max_spp, float target_history) {
    if (base_spp < 2u || !budget_pow2(base_spp)) return BudgetParams::BASE;
    if (max_spp < base_spp || !budget_pow2(max_spp)) return BudgetParams::MAX;
    if (!(std::isfinite(target_history) && target_history >= 1.0f)) return BudgetParams::TARGET;
    return BudgetParams::OK;
}

// how a mi355pt_budget_motion carries a pixel, or what is wrong with it before the form's own pointer rules (api_checks.hpp motion_verdict,
// flow_checks.hpp flow_in_verdict) are asked.  A struct without a table and without records must be all zero
enum class BudgetCarry { STATIC, TABLE, FLOW, BOTH, IDS_ALONE };
inline BudgetCarry budget_carry_verdict(const void* ids_cur, const void* ids_prev, const void* table, uint32_t n_entries, const void* flow) {
    if (table && flow) return BudgetCarry::BOTH;
    if (table) return BudgetCarry::TABLE;
    if (flow) return BudgetCarry::FLOW;
    return ids_cur || ids_prev || n_entries ? BudgetCarry::IDS_ALONE : BudgetCarry::STATIC;
}

// The formula of the header: base_spp << j, j the smallest integer >= 0 with (lmin + 1) 2^j >= target or base_spp << j == max_spp.
// lmin + 1 is rounded once; a doubling is exact (an overflow gives +inf, which ends the loop).  lmin is >= 0 or +inf, never a NaN (the
// probe's minimum); base_spp and max_spp are powers of two, base_spp <= max_spp: at most 31 turns
PT_BUDGET_HD inline uint32_t budget_spp(float lmin, uint32_t base_spp, uint32_t max_spp, float target_history) {
    float reach = lmin + 1.0f;
    uint32_t n = base_spp;
    while (n < max_spp && !(reach >= target_history)) {
        reach = reach * 2.0f;
        n <<= 1;
    }
    return n;
}

// a tile's count as the driver takes it: clamped into [base_spp, max_spp], never trusted
PT_BUDGET_HD inline uint32_t budget_clamp(uint32_t n, uint32_t base_spp, uint32_t max_spp) { return n < base_spp ? base_spp : (n > max_spp ? max_spp : n); }

// the count a tile ends the driver with: the smallest base_spp << j that is >= the clamped count (the count itself when it is a power of two)
inline uint32_t budget_rendered(uint32_t n, uint32_t base_spp, uint32_t max_spp) {
    const uint32_t c = budget_clamp(n, base_spp, max_spp);
    uint32_t level = base_spp;
    while (level < c) level <<= 1;
    return level;
}

// the length credit of a tile with count n: (float)(n / base_spp - 1) where n > base_spp, else no credit (the tile is not written)
inline bool budget_has_credit(uint32_t n, uint32_t base_spp) { return n > base_spp; }
inline float budget_credit(uint32_t n, uint32_t base_spp) { return (float)(n / base_spp - 1u); }

}  // namespace pt
