// Runs a wave's tail-queue schedule on csrc/tail_queue_plan.hpp (host only) the way pt_kernel_body.inc does — front, push, pass — for
// seeded random sequences biased towards the real ones, and checks the properties the kernels rely on.  tests/test_tail_queue_plan.py.
//   usage: tail_queue_plan_check <two_queues 0|1> <capacity per queue> <seed> <work items>
//   prints one line "ok pushes pops passes max1 max2 max_total fresh_passes drain_passes"; exits 1 with a message at the first violation
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "tail_queue_plan.hpp"

using namespace pt;

static void fail(const char* what, long a = 0, long b = 0) {
    std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
    std::exit(1);
}
#define CHECK(c, ...) do { if (!(c)) fail(#c, ##__VA_ARGS__); } while (0)

struct Queue {
    uint32_t count = 0;                  // the kernel's wave-uniform count
    std::vector<long> slot;              // record id in each slot, -1 = free (the memory)
    std::vector<long> order;             // the model: ids waiting, oldest first (knows nothing of slots)
    explicit Queue(uint32_t cap) : slot(cap, -1) {}
};

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const bool two = std::atoi(argv[1]) != 0;
    const uint32_t cap = (uint32_t)std::atoi(argv[2]), seed = (uint32_t)std::atoi(argv[3]);
    const int n_items = std::atoi(argv[4]);
    const uint32_t MIN = 64;             // PT_TAILQ_MIN: a pass starts when a whole wave waits
    std::mt19937 rng(seed);
    auto uni = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1u)); };
    auto coin = [&](double p) { return (rng() >> 8) * (1.0 / 16777216.0) < p; };
    long next_id = 0, pushes = 0, pops = 0, passes = 0, fresh_passes = 0, drain_passes = 0;
    uint32_t max1 = 0, max2 = 0, max_total = 0;
    std::vector<char> popped_once;

    for (int item = 0; item < n_items; ++item) {
        Queue q1(cap), q2(cap);
        // the item's character: how many of the lanes that traced go on (the real ones: ~43 of 64 after a continuing iteration, ~58 after a
        // camera iteration), the share of class 2, the pool (0 .. a few thousand pairs; a pool smaller than a wave: drain passes only)
        const int kind = (int)uni(0, 5);
        const double p_on = kind == 0 ? 0.97 : kind == 1 ? 0.0 : kind == 2 ? 0.9 : 0.67;
        const double p_cls2 = !two ? 0.0 : (kind == 3 ? 1.0 : kind == 4 ? 0.5 : kind == 5 ? 0.1 : 0.3);
        long pool = kind == 1 ? (long)uni(0, 200) : coin(0.2) ? (long)uni(0, 63) : (long)uni(64, 4096);
        uint32_t active = 0;             // lanes that carry a path into this iteration's traversal
        for (long iter = 0;; ++iter) {
            CHECK(iter < 1000000, iter);
            const bool draining_before = pool == 0;
            // free lanes take new paths from the pool
            const uint32_t n_new = (uint32_t)std::min<long>(64 - active, pool);
            pool -= n_new; active += n_new;
            const bool draining = pool == 0;
            if (active == 0 && draining && q1.count == 0 && q2.count == 0) break;
            // front: every lane that traced ends its path or goes on; the ones that go on push a record.  While draining, paths end a little
            // more often than not so that the item ends.
            // Now and then every lane goes on at once (the largest push).
            uint32_t k1 = 0, k2 = 0;
            const double p_iter = draining_before ? std::min(p_on, 0.8) : coin(0.05) ? 1.0 : p_on;
            for (uint32_t l = 0; l < active; ++l)
                if (coin(p_iter)) { if (coin(p_cls2)) ++k2; else ++k1; }
            Queue* qs[2] = {&q1, &q2};
            const uint32_t ks[2] = {k1, k2};
            for (int c = 0; c < 2; ++c) {
                Queue& q = *qs[c];
                for (uint32_t r = 0; r < ks[c]; ++r) {
                    const uint32_t s = tq_push_slot(q.count, r);
                    CHECK(s < cap, s, cap);                                   // no slot index reaches the capacity
                    CHECK(q.slot[s] < 0, s, q.slot[s]);                        // no live slot is overwritten
                    if (r) CHECK(s == tq_push_slot(q.count, r - 1) + 1u, s);   // consecutive ranks, consecutive slots
                    q.slot[s] = next_id; q.order.push_back(next_id); popped_once.push_back(0); ++next_id; ++pushes;
                }
                q.count += ks[c];
                CHECK(q.count == q.order.size(), q.count);
            }
            active = 0;                                                        // pushed or ended: every lane is free after the front
            max1 = std::max(max1, q1.count); max2 = std::max(max2, q2.count); max_total = std::max(max_total, q1.count + q2.count);
            if (two) CHECK(q1.count + q2.count <= 191u, q1.count, q2.count); else CHECK(q1.count <= 127u && q2.count == 0u, q1.count, q2.count);
            // the pass.  All 64 lanes are free in the kernel; the drain phase also runs with fewer (1 .. 64) — the functions do not assume it
            const uint32_t n_free = draining && coin(0.5) ? uni(1, 64) : 64u;
            const bool due = tq_pass_due(q1.count, q2.count, draining, two, MIN);
            CHECK(due == ((two && q2.count >= MIN) || q1.count >= MIN || (draining && q1.count + q2.count != 0u)), q1.count, q2.count);
            if (!due) continue;
            const TqTake tk = tq_pass_take(q1.count, q2.count, n_free, draining, two, MIN);
            ++passes; if (draining) ++drain_passes;
            CHECK(tk.n1 <= q1.count && tk.n2 <= q2.count && tk.n1 + tk.n2 <= n_free, tk.n1, tk.n2);
            CHECK(tk.n1 + tk.n2 > 0u, q1.count, q2.count);
            if (!two) CHECK(tk.n2 == 0u, tk.n2);
            if (!draining) {
                // one class per pass while new paths arrive, the class with its own queue first, and a full wave of it
                CHECK(tk.n1 == 0u || tk.n2 == 0u, tk.n1, tk.n2);
                if (q2.count >= MIN) CHECK(tk.n2 == MIN && tk.n1 == 0u, tk.n1, tk.n2); else CHECK(tk.n1 == MIN, tk.n1, tk.n2);
            } else {
                // draining: whatever waits shares the pass, queue 2 first — unless queue 1 alone holds a whole wave and queue 2 does not
                const bool only1 = q1.count >= MIN && q2.count < MIN;
                const uint32_t want2 = only1 ? 0u : std::min(n_free, q2.count);
                CHECK(tk.n2 == want2 && tk.n1 == std::min(n_free - want2, q1.count), tk.n1, tk.n2);
            }
            const uint32_t ns[2] = {tk.n1, tk.n2};
            bool fresh = false;
            for (int c = 0; c < 2; ++c) {
                Queue& q = *qs[c];
                const uint32_t n = ns[c];
                uint32_t just = 0;                                             // records of this pass that THIS iteration's front pushed
                for (uint32_t r = 0; r < n; ++r) {
                    const uint32_t s = tq_pop_slot(q.count, n, r);
                    CHECK(s < cap, s, cap);
                    CHECK(q.slot[s] >= 0, s);                                  // a live record
                    if (r) CHECK(s == tq_pop_slot(q.count, n, r - 1) + 1u, s);
                    const long id = q.slot[s];
                    CHECK(!popped_once[id], id); popped_once[id] = 1; ++pops;
                    // the model: the n newest records of the queue, whatever the slots
                    CHECK(id == q.order[q.order.size() - n + r], id, r);
                    if (id >= next_id - (long)(k1 + k2)) ++just;
                    q.slot[s] = -1;
                }
                // locality: the records pushed a moment ago go first — all of them, or a whole pass of them — before any older one
                if (n) { CHECK(just == std::min(ks[c], n), just, n); if (just) fresh = true; }
                q.order.resize(q.order.size() - n);
                q.count -= n;
            }
            if (fresh) ++fresh_passes;
            // the popped paths are shaded and trace their next ray in the lanes that took them
            active = tk.n1 + tk.n2;
        }
        CHECK(q1.count == 0u && q2.count == 0u && q1.order.empty() && q2.order.empty(), q1.count, q2.count);   // empty between work items
        for (uint32_t s = 0; s < cap; ++s) CHECK(q1.slot[s] < 0 && q2.slot[s] < 0, s);
    }
    CHECK(pushes == pops, pushes, pops);
    for (long id = 0; id < next_id; ++id) CHECK(popped_once[id] == 1, id);
    std::printf("ok %ld %ld %ld %u %u %u %ld %ld\n", pushes, pops, passes, max1, max2, max_total, fresh_passes, drain_passes);
    return 0;
}
