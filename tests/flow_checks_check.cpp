// TEST INFRASTRUCTURE ONLY: walks the pure predicates of csrc/flow_checks.hpp (the argument checks of include/mi355pt_flow.h) with a plain
// C++ compiler — no HIP, no device — and, built a second time, under ASan + UBSan (tests/test_flow.py).  Pointers are only compared and
// tested for alignment, never dereferenced: the buffers behind them are real so that the sanitizers see nothing invented.
//   flow_checks_check <seed> <n>      n random argument sets on top of the fixed ones; prints "ok <checks>" and exits 0
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "flow_checks.hpp"

using namespace pt;

static unsigned long g_checks = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

static uint32_t rnd(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

int main(int argc, char** argv) {
    uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    const long n = argc > 2 ? std::strtol(argv[2], nullptr, 10) : 0;
    alignas(64) static unsigned char pool[1024];
    void* const a16 = pool + 64;           // 16-byte aligned
    void* const odd = pool + 68;           // 4-byte aligned only
    void* const ids = pool + 256;
    void* const idp = pool + 512;
    void* const out = pool + 768;

    // the flow pass's outputs: the first verdict that applies, in the header's order
    CHECK(flow_out_verdict(nullptr, 16, nullptr) == FlowOut::MISSING);
    CHECK(flow_out_verdict(nullptr, 16, ids) == FlowOut::MISSING);
    CHECK(flow_out_verdict(odd, 16, nullptr) == FlowOut::MISALIGNED);
    CHECK(flow_out_verdict(odd, 16, odd) == FlowOut::MISALIGNED);            // misaligned comes before "the same buffer"
    CHECK(flow_out_verdict(odd, 1, nullptr) == FlowOut::OK);                 // the host form asks for no alignment
    CHECK(flow_out_verdict(odd, 1, odd) == FlowOut::SAME_BUFFER);
    CHECK(flow_out_verdict(a16, 16, a16) == FlowOut::SAME_BUFFER);
    CHECK(flow_out_verdict(a16, 16, nullptr) == FlowOut::OK);
    CHECK(flow_out_verdict(a16, 16, ids) == FlowOut::OK);

    // the accumulation's inputs
    const void* outs[4] = {out, nullptr, (unsigned char*)out + 64, nullptr};
    CHECK(flow_in_verdict(ids, idp, nullptr, 16, outs, 4) == FlowIn::MISSING);
    CHECK(flow_in_verdict(nullptr, nullptr, nullptr, 16, outs, 4) == FlowIn::MISSING);
    CHECK(flow_in_verdict(ids, idp, odd, 16, outs, 4) == FlowIn::MISALIGNED);
    CHECK(flow_in_verdict(ids, idp, odd, 1, outs, 4) == FlowIn::OK);
    CHECK(flow_in_verdict(nullptr, idp, a16, 16, outs, 4) == FlowIn::PREV_IDS_ALONE);
    CHECK(flow_in_verdict(nullptr, nullptr, a16, 16, outs, 4) == FlowIn::OK);          // no ids at all: allowed
    CHECK(flow_in_verdict(ids, nullptr, a16, 16, outs, 4) == FlowIn::OK);
    CHECK(flow_in_verdict(ids, idp, a16, 16, outs, 4) == FlowIn::OK);
    CHECK(flow_in_verdict(ids, idp, a16, 16, outs, 0) == FlowIn::OK);
    for (int k = 0; k < 4; ++k) {
        for (const void* alias : {(const void*)a16, (const void*)ids, (const void*)idp}) {
            const void* o[4] = {out, nullptr, (unsigned char*)out + 64, nullptr};
            o[k] = alias;
            CHECK(flow_in_verdict(ids, idp, a16, 16, o, 4) == FlowIn::ALIASES_OUTPUT);
        }
    }
    // a null output never aliases a null id pointer
    CHECK(flow_in_verdict(nullptr, nullptr, a16, 16, outs, 4) == FlowIn::OK);

    // random argument sets against the rule written out once more
    std::vector<void*> cands = {nullptr, a16, odd, ids, idp, out, pool + 16, pool + 17, pool + 32};
    for (long i = 0; i < n; ++i) {
        const void* fl = cands[rnd(seed) % cands.size()];
        const void* ic = cands[rnd(seed) % cands.size()];
        const void* ip = cands[rnd(seed) % cands.size()];
        const size_t align = (rnd(seed) & 1u) ? 16 : 1;
        const void* o[4];
        for (auto& x : o) x = cands[rnd(seed) % cands.size()];
        FlowIn want = FlowIn::OK;
        bool alias = false;
        for (const void* x : o) alias = alias || (x && (x == fl || x == ic || x == ip));
        if (!fl) want = FlowIn::MISSING;
        else if (((uintptr_t)fl & (align - 1)) != 0) want = FlowIn::MISALIGNED;
        else if (ip && !ic) want = FlowIn::PREV_IDS_ALONE;
        else if (alias) want = FlowIn::ALIASES_OUTPUT;
        CHECK(flow_in_verdict(ic, ip, fl, align, o, 4) == want);
        FlowOut wo = !fl ? FlowOut::MISSING : (((uintptr_t)fl & (align - 1)) != 0) ? FlowOut::MISALIGNED : fl == ic ? FlowOut::SAME_BUFFER : FlowOut::OK;
        CHECK(flow_out_verdict(fl, align, ic) == wo);
    }
    std::printf("ok %lu\n", g_checks);
    return 0;
}
