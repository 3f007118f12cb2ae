// The staging arithmetic of csrc/tail_queue_plan.hpp (host only): the kernels with one tail queue keep the records a pass takes in the same
// iteration in LDS.  Enumerates every count waiting before the push (0 .. 127), every number of pushing lanes (0 .. 64) and draining
// on / off, runs the front's push and the pass twice — once with everything in the global stack (tq_push_slot / tq_pass_take / tq_pop_slot,
// the reference) and once with the staging functions on a model of the LDS area — and checks that the two hand the same record to the same
// lane.  Then replays the steady cadence of the benchmark's kernel and reports the share of records staged.  tests/test_tail_queue_stage.py.
//   usage: tail_queue_stage_check
//   prints one line "ok cases staged_cases cadence_pushes cadence_staged"; exits 1 with a message at the first violation
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

int main() {
    const uint32_t MIN = 64u;            // PT_TAILQ_MIN
    const uint32_t N_FREE = 64u;         // every lane is free after the front (pt_kernel_body.inc)
    const uint32_t CAP1 = 128u;          // PT_TAILQ_RING1: the one-queue stack's capacity
    static_assert(TQ_STAGE_SLOTS == 64u, "one push");
    long cases = 0, staged_cases = 0;
    for (uint32_t q0 = 0; q0 < 128u; ++q0)
        for (uint32_t p = 0; p <= 64u; ++p)
            for (int dr = 0; dr < 2; ++dr) {
                const bool draining = dr != 0;
                ++cases;
                // record ids: the q0 older ones are 0 .. q0-1 in their slots, this iteration's pushes are q0 + rank
                // reference: everything in the global stack
                std::vector<long> ref(q0 + p);
                for (uint32_t s = 0; s < q0; ++s) ref[s] = (long)s;
                for (uint32_t r = 0; r < p; ++r) ref[tq_push_slot(q0, r)] = (long)(q0 + r);
                const uint32_t count = q0 + p;
                const bool due = tq_pass_due(count, 0u, draining, false, MIN);
                const bool stage = tq_stage_pushes(q0, p, draining, MIN);
                CHECK(stage == (p != 0u && due), q0, p, dr);
                if (!due) {
                    CHECK(!stage, q0, p, dr);
                    continue;
                }
                const TqTake tk = tq_pass_take(count, 0u, N_FREE, draining, false, MIN);
                CHECK(tk.n2 == 0u && tk.n1 == std::min(N_FREE, count), tk.n1, tk.n2);
                const uint32_t n = tk.n1;
                if (!stage) {
                    // nothing staged: every slot the pass hands out is the reference's and lies in the global stack
                    for (uint32_t r = 0; r < n; ++r) {
                        const TqStagePop sp = tq_stage_pop(count, 0u, n, r);
                        CHECK(!sp.staged && sp.slot == tq_pop_slot(count, n, r), q0, p, r);
                    }
                    continue;
                }
                ++staged_cases;
                // staged: the older records in the global stack, this iteration's in the LDS model
                std::vector<long> glob(q0), lds(TQ_STAGE_SLOTS, -1);
                for (uint32_t s = 0; s < q0; ++s) glob[s] = (long)s;
                for (uint32_t r = 0; r < p; ++r) {
                    const uint32_t i = tq_stage_push_index(r);
                    CHECK(i < TQ_STAGE_SLOTS, i, r);                               // inside the LDS area
                    CHECK(lds[i] < 0, i, r);                                       // distinct
                    lds[i] = (long)(q0 + r);
                }
                uint32_t from_lds = 0;
                for (uint32_t r = 0; r < n; ++r) {
                    const TqStagePop sp = tq_stage_pop(q0, p, n, r);
                    CHECK(sp.slot == tq_pop_slot(count, n, r), q0, p, r);          // the slot today's arithmetic gives this lane
                    long id;
                    if (sp.staged) {
                        CHECK(sp.slot >= q0 && sp.index < TQ_STAGE_SLOTS && sp.index < p, sp.slot, sp.index, p);
                        id = lds[sp.index];
                        CHECK(id >= 0, sp.index, r);                               // a staged record, taken once
                        lds[sp.index] = -1;
                        ++from_lds;
                    } else {
                        CHECK(sp.slot < q0, sp.slot, q0);
                        id = glob[sp.slot];
                        if (q0 <= 63u) CHECK(sp.slot < CAP1, sp.slot);
                    }
                    CHECK(id == ref[sp.slot], id, ref[sp.slot], r);                // the same record reaches the same lane
                }
                // the pass takes every staged record: none is left in LDS, and the global stack below the pre-push count is all that remains
                CHECK(from_lds == p, from_lds, p);
                for (uint32_t i = 0; i < TQ_STAGE_SLOTS; ++i) CHECK(lds[i] < 0, i);
                CHECK(count - n <= q0, count - n, q0);
            }
    // the steady cadence of the benchmark's kernel (scene 3, MIS): a wave that took 64 queued paths pushes about 43 records after the next
    // traversal, a wave of 64 fresh camera paths about 62; a pass pops 64 whenever 64 wait
    long pushes = 0, staged = 0;
    uint32_t q = 0;
    bool had_pass = false;
    for (int iter = 0; iter < 100000; ++iter) {
        const uint32_t p = had_pass ? 43u : 62u;
        const bool stage = tq_stage_pushes(q, p, false, MIN);
        pushes += p;
        if (stage) staged += p;
        q += p;
        CHECK(q <= 127u, q);
        had_pass = tq_pass_due(q, 0u, false, false, MIN);
        CHECK(stage == had_pass, iter);
        if (had_pass) q -= tq_pass_take(q, 0u, N_FREE, false, false, MIN).n1;
    }
    std::printf("ok %ld %ld %ld %ld\n", cases, staged_cases, pushes, staged);
    return 0;
}
