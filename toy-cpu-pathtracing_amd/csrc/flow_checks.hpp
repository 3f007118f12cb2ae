// The pure predicates of api_flow.cpp's argument checks (include/mi355pt_flow.h), beside api_checks.hpp's, whose misaligned() and output_is_one_of() they use.
// Host arithmetic only, no HIP: compiles with a plain C++ compiler (tests/flow_checks_check.cpp walks them, plain and under ASan + UBSan).
// They answer with a verdict; the refusal's code and text stay at the caller's fail(...).
#pragma once
#include <cstddef>
#include <cstdint>

#include "api_checks.hpp"

namespace pt {

// what is wrong with the output buffers of a flow pass: the first that applies, in this order.  ids may be null (not wanted)
enum class FlowOut { OK, MISSING, MISALIGNED, SAME_BUFFER };
inline FlowOut flow_out_verdict(const void* flow, size_t flow_align, const void* ids) {
    if (!flow) return FlowOut::MISSING;
    if (misaligned(flow, flow_align)) return FlowOut::MISALIGNED;
    if (flow == ids) return FlowOut::SAME_BUFFER;
    return FlowOut::OK;
}

// what is wrong with the records and the id buffers of a flow-aware accumulation: the first that applies, in this order.  ids_cur may be
// null when ids_prev is; `outs`: the call's n_outs output pointers (null ones among them) and, for the rectified form, its scratch
enum class FlowIn { OK, MISSING, MISALIGNED, PREV_IDS_ALONE, ALIASES_OUTPUT };
inline FlowIn flow_in_verdict(const void* ids_cur, const void* ids_prev, const void* flow, size_t flow_align, const void* const* outs, int n_outs) {
    if (!flow) return FlowIn::MISSING;
    if (misaligned(flow, flow_align)) return FlowIn::MISALIGNED;
    if (ids_prev && !ids_cur) return FlowIn::PREV_IDS_ALONE;
    return output_is_one_of(outs, n_outs, flow, ids_cur, ids_prev) ? FlowIn::ALIASES_OUTPUT : FlowIn::OK;
}

}  // namespace pt
