// The tail queue's index arithmetic (pt_kernel.hpp TAIL QUEUE, pt_kernel_body.inc): which slot a push writes, which slots a pass reads and
// how many records a pass takes from each of a wave's queues.  Plain integer functions of the wave-uniform counts — no HIP, no state — so
// that tests/test_tail_queue_plan.py runs a wave's schedule on them without a GPU (constexpr: callable from the kernels as they stand).
//
// Each queue is a STACK: `count` records wait in slots [0, count).  A push of n records writes slots [count, count + n), a pass that takes
// n reads slots [count - n, count) — the newest, which the front of the vertex stored a few hundred instructions earlier and which are
// still in the L2; the bottom of the stack goes cold until the work item drains.  Consecutive ranks map to consecutive slots in both
// directions: with the field-major layout of the records every store / load instruction of a wave covers whole 128-byte lines.
//
// Occupancy: a pass starts as soon as a queue holds pass_min (64) records, takes min(free lanes, count) and every lane is free after the
// front, so a queue holds at most 63 after a pass and an iteration adds at most 64: with one queue count <= 127; with two, a pass empties
// one of them to <= 63 while the other stays below 64, so both together hold <= 63 + 63 + 64 = 190 (the capacities: 128 and 2 x 256).
#pragma once
#include <cstdint>

namespace pt {

// slot of the record pushed by the lane of rank `rank` among the pushing lanes, `count` records waiting before the push
constexpr uint32_t tq_push_slot(uint32_t count, uint32_t rank) { return count + rank; }
// slot read by the lane of rank `rank` among the n lanes that take from a queue of `count` records (n <= count, rank < n)
constexpr uint32_t tq_pop_slot(uint32_t count, uint32_t n, uint32_t rank) { return count - n + rank; }

struct TqTake { uint32_t n1, n2; };      // records a pass takes from queue 1 (every other class) and queue 2 (the class with its own queue)

// Is a pass due?  When a queue is full (pass_min records: a whole wave), or when the work item has no new paths left (`draining`) and
// anything waits at all.  c2 is 0 in the kernels with one queue.
constexpr bool tq_pass_due(uint32_t c1, uint32_t c2, bool draining, bool two_queues, uint32_t pass_min) {
    return (two_queues && c2 >= pass_min) || c1 >= pass_min || (draining && (c1 | c2) != 0u);
}
// What the pass takes, n_free lanes being free: ONE class while new paths still arrive — queue 2 first —, and when the work item is
// draining, whatever waits in either queue shares the pass (the first n2 free lanes take from queue 2, the next n1 from queue 1).
constexpr TqTake tq_pass_take(uint32_t c1, uint32_t c2, uint32_t n_free, bool draining, bool two_queues, uint32_t pass_min) {
    const bool full2 = two_queues && c2 >= pass_min, full1 = c1 >= pass_min;
    const uint32_t n2 = (full2 || (draining && !full1)) ? (n_free < c2 ? n_free : c2) : 0u;
    const uint32_t n1 = (!full2 || draining) ? (n_free - n2 < c1 ? n_free - n2 : c1) : 0u;
    return TqTake{n1, n2};
}

// ---- staging (the kernels with ONE queue) ----
// When a pass follows the front in the same iteration it takes the newest min(64, count) records, and those include every record the front
// has just pushed (<= 64, every lane being free after the front).  Such records never need the global stack: the front writes them to LDS
// instead (the traversal stack, idle between two traversals), rank r of the pushing lanes at LDS index r, and the pass reads them from
// there.  Logically they still sit in slots [count, count + n_push) of the stack: the pass hands out the slots tq_pop_slot names, a slot at
// or above the pre-push count comes from LDS, one below it from the global stack, and the count ends where it ends without staging.
constexpr uint32_t TQ_STAGE_SLOTS = 64u;          // records the LDS area holds: one push

// Does this iteration stage its pushes?  `count`: records waiting before the push; n_push: lanes that push (<= 64).  Exactly when a pass is
// due after the push — that pass takes all of them.
constexpr bool tq_stage_pushes(uint32_t count, uint32_t n_push, bool draining, uint32_t pass_min) {
    return n_push != 0u && tq_pass_due(count + n_push, 0u, draining, false, pass_min);
}
// LDS index of the record staged by the lane of rank `rank` among the pushing lanes
constexpr uint32_t tq_stage_push_index(uint32_t rank) { return rank; }

struct TqStagePop { uint32_t slot; bool staged; uint32_t index; };    // the logical stack slot; in LDS?; if so, at which index
// What the lane of rank `rank` among the n_take lanes of the pass pops, the iteration having staged n_push records on top of `count` waiting
// ones (n_push = 0: nothing staged, every slot is in the global stack)
constexpr TqStagePop tq_stage_pop(uint32_t count, uint32_t n_push, uint32_t n_take, uint32_t rank) {
    const uint32_t slot = tq_pop_slot(count + n_push, n_take, rank);
    return TqStagePop{slot, slot >= count, slot >= count ? slot - count : 0u};
}

// ---- the light-hit queue (the kernels with ONE tail queue; pt_kernel.hpp LIGHT-HIT QUEUE) ----
// A second stack of the wave, for the paths whose hit is on an emitter: they end there, and what is left of them — the emitter's radiance
// with the strategy's weight, the film — is computed 64 at a time.  Same arithmetic as the tail queue's: `count` records wait in slots
// [0, count), the pushing lanes write consecutive slots on top by rank, a pass pops the newest min(64, count) by rank.  A pass is due as
// soon as 64 wait — the front has just pushed and every lane is free — so at most 63 stay behind and an iteration adds at most 64: the
// count never exceeds LQ_MAX_WAITING, inside the LQ_SLOTS of the stack.  When the work item is done (its pool spent, no lane active, the
// tail queue empty) one last pass takes what is left, fewer than 64.
constexpr uint32_t LQ_SLOTS = 128u;               // entries of the stack
constexpr uint32_t LQ_PASS = 64u;                 // records a full pass takes: one per lane
constexpr uint32_t LQ_MAX_WAITING = 127u;         // the bound of the count
constexpr uint32_t lq_push_slot(uint32_t count, uint32_t rank) { return count + rank; }
constexpr bool lq_pass_due(uint32_t count, bool item_done) { return count >= LQ_PASS || (item_done && count != 0u); }
constexpr uint32_t lq_pass_take(uint32_t count) { return count < LQ_PASS ? count : LQ_PASS; }
// slot popped by lane `rank` of the n = lq_pass_take(count) lanes of the pass
constexpr uint32_t lq_pop_slot(uint32_t count, uint32_t n, uint32_t rank) { return count - n + rank; }

}  // namespace pt
