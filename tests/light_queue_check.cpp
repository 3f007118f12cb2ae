// The light-hit queue's index arithmetic of csrc/tail_queue_plan.hpp (host only; lq_push_slot, lq_pass_due, lq_pass_take, lq_pop_slot): the
// kernels with one tail queue push the paths that arrive at an emitter to a stack of the wave and evaluate them 64 at a time.  Enumerates
// every count waiting (0 .. 127) and every number of pushing lanes (0 .. 64) on a model of the stack that holds record ids, in the order of
// pt_kernel_body.inc: a pass whenever one is due, the front's push, a pass if one is due, and the pass at the end of the work item.  Then
// replays a long random schedule.  tests/test_light_queue.py.
//   usage: light_queue_check
//   prints one line "ok cases passes max_count"; exits 1 with a message at the first violation
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tail_queue_plan.hpp"

using namespace pt;

static void fail(const char* what, long a = 0, long b = 0, long c = 0) {
    std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
    std::exit(1);
}
#define CHECK(c, ...) do { if (!(c)) fail(#c, ##__VA_ARGS__); } while (0)

struct Stack {
    std::vector<long> slot = std::vector<long>(LQ_SLOTS, -1);    // record id per slot, -1: empty
    uint32_t count = 0;
    long next_id = 0, passes = 0;
    uint32_t max_count = 0;

    void fill(uint32_t n) { for (uint32_t s = 0; s < n; ++s) slot[s] = next_id++; count = n; }
    // the front's push: p lanes, ranks 0 .. p-1
    void push(uint32_t p) {
        for (uint32_t r = 0; r < p; ++r) {
            const uint32_t s = lq_push_slot(count, r);
            CHECK(s < LQ_SLOTS, s, count, r);                                   // inside the stack
            CHECK(s == count + r, s, count, r);                                 // consecutive ranks, consecutive slots, on top
            CHECK(slot[s] < 0, s, count, r);                                    // distinct, and no waiting record overwritten
            slot[s] = next_id++;
        }
        count += p;
        CHECK(count <= LQ_MAX_WAITING, count, p);
        max_count = std::max(max_count, count);
    }
    // a pass: lanes 0 .. n-1 pop; returns n
    uint32_t pass() {
        const uint32_t n = lq_pass_take(count);
        CHECK(n == std::min(64u, count) && n <= LQ_PASS, n, count);
        long newest = -1;
        for (uint32_t s = 0; s < LQ_SLOTS; ++s) newest = std::max(newest, slot[s]);
        std::vector<long> got;
        for (uint32_t r = 0; r < n; ++r) {
            const uint32_t s = lq_pop_slot(count, n, r);
            CHECK(s < LQ_SLOTS && s >= count - n && s < count, s, count, r);
            CHECK(slot[s] >= 0, s, count, r);                                   // a waiting record, taken once
            got.push_back(slot[s]);
            slot[s] = -1;
        }
        // exactly the newest n: every id left is older than every id taken
        if (n != 0u) {
            const long oldest_taken = *std::min_element(got.begin(), got.end());
            CHECK(*std::max_element(got.begin(), got.end()) == newest, newest, n);
            for (uint32_t s = 0; s < LQ_SLOTS; ++s) CHECK(slot[s] < oldest_taken, s, slot[s], oldest_taken);
        }
        count -= n;
        for (uint32_t s = 0; s < LQ_SLOTS; ++s) CHECK((slot[s] >= 0) == (s < count), s, count);   // what waits is slots [0, count)
        ++passes;
        return n;
    }
};

int main() {
    static_assert(LQ_SLOTS == 128u && LQ_PASS == 64u && LQ_MAX_WAITING == 127u && LQ_MAX_WAITING < LQ_SLOTS, "the bound lies inside the stack");
    long cases = 0, passes = 0;
    uint32_t max_count = 0;
    for (uint32_t q0 = 0; q0 < 128u; ++q0)
        for (uint32_t p = 0; p <= 64u; ++p) {
            ++cases;
            Stack st;
            st.fill(q0);
            // a pass is due exactly from 64 records on; the kernel runs it right after the push that made it due, before anything else is pushed
            CHECK(lq_pass_due(q0, false) == (q0 >= 64u), q0);
            if (lq_pass_due(q0, false)) CHECK(st.pass() == 64u, q0);
            CHECK(!lq_pass_due(st.count, false) && st.count <= 63u, st.count);
            st.push(p);
            if (lq_pass_due(st.count, false)) CHECK(st.pass() == 64u, q0, p);
            CHECK(!lq_pass_due(st.count, false) && st.count <= 63u, st.count);
            // the end of the work item: one last pass takes whatever is left, fewer than 64, and empties the stack
            CHECK(lq_pass_due(st.count, true) == (st.count != 0u), st.count);
            if (lq_pass_due(st.count, true)) { const uint32_t left = st.count; CHECK(st.pass() == left && left < 64u, left); }
            CHECK(st.count == 0u && !lq_pass_due(st.count, true), st.count);
            passes += st.passes;
            max_count = std::max(max_count, st.max_count);
        }
    // a long schedule of random pushes (a small generator of its own: the same on every host), with an item's end now and then
    Stack st;
    uint32_t x = 12345u;
    for (int iter = 0; iter < 200000; ++iter) {
        x = x * 1664525u + 1013904223u;
        const uint32_t p = ((x >> 24) & 1u) ? (x >> 16) % 65u : (x >> 16) % 4u;     // mostly a lane or two, sometimes many
        st.push(p);
        const bool item_done = ((x >> 8) & 255u) == 0u;
        if (lq_pass_due(st.count, item_done)) st.pass();
        // (64 or more waited when the item ended: the pass took 64, and the loop's exit condition sees the rest — one more iteration, without
        // rays or pushes, whose pass takes them)
        if (item_done && st.count != 0u) { CHECK(lq_pass_due(st.count, true), st.count); st.pass(); }
        CHECK(st.count <= 63u && (!item_done || st.count == 0u), st.count);
    }
    passes += st.passes;
    max_count = std::max(max_count, st.max_count);
    std::printf("ok %ld %ld %u\n", cases, passes, max_count);
    return 0;
}
