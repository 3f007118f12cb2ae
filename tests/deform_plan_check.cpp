// TEST INFRASTRUCTURE ONLY.  csrc/deform_plan.hpp on its own (plain g++, no HIP):
//   - the layout of seeded scenes: every given array of every updated mesh has its own range of the staging buffer, the ranges are disjoint,
//     in the updates' order and add up to staging_floats, which never exceeds deform_staging_capacity; an array that is not given has no
//     range; every slot names its mesh's range of the index pool and its counts;
//   - the per-instance table and the moved mask: an instance has a slot exactly when its mesh is updated, and it is that mesh's;
//   - the table the device reads: the instance words, the slot records at a multiple of four words, padding filled with DEFORM_NO_SLOT;
//   - a gather through the table on the host — what deform_tris_kernel does, restated here — lands on the values the update holds;
//   - refusals: an id out of range, ids not ascending or repeated, counts that differ from the mesh's, a short offset table;
//   - the "same bytes" test: null = same, equal bytes, one flipped bit, -0.0 against +0.0, zero length.
// usage: deform_plan_check <seed> <n_meshes>   ->   "ok <n_meshes>"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "deform_plan.hpp"

using namespace pt;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

namespace {
std::mt19937 rng;
uint32_t below(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; }
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: deform_plan_check <seed> <n_meshes>\n"); return 2; }
    rng.seed((uint32_t)std::atoi(argv[1]));
    const size_t n_meshes = (size_t)std::atoi(argv[2]);

    // ---- the "same bytes" test ----
    {
        float a[4] = {1.0f, -0.0f, 3.5f, 7.0f}, b[4] = {1.0f, -0.0f, 3.5f, 7.0f};
        CHECK(deform_same_bytes(nullptr, a, 4) && deform_same_bytes(a, b, 4) && deform_same_bytes(a, b, 0));
        b[1] = 0.0f;
        CHECK(!deform_same_bytes(a, b, 4) && deform_same_bytes(a, b, 1));
        b[1] = -0.0f;
        uint32_t w; std::memcpy(&w, &b[3], 4); w ^= 1u; std::memcpy(&b[3], &w, 4);
        CHECK(!deform_same_bytes(a, b, 4) && deform_same_bytes(a, b, 3));
    }
    CHECK(deform_table_slots_at(0) == 0 && deform_table_slots_at(1) == 4 && deform_table_slots_at(4) == 4 && deform_table_slots_at(5) == 8);
    if (n_meshes == 0) {
        DeformPlan plan;
        const std::vector<uint32_t> off = deform_index_offsets(nullptr, 0);
        CHECK(off.size() == 1 && off[0] == 0);
        CHECK(make_deform_plan(nullptr, 0, nullptr, nullptr, 0, off, nullptr, 0, &plan) && plan.slots.empty() && plan.staging_floats == 0);
        CHECK(deform_table(plan).empty());
        std::printf("ok 0\n");
        return 0;
    }

    // ---- a seeded scene: meshes of 1 .. 40 triangles, 1 .. 3 n_meshes instances, every subset size of updates ----
    std::vector<uint32_t> nv(n_meshes), nt(n_meshes);
    for (size_t g = 0; g < n_meshes; ++g) { nv[g] = 3 + below(60); nt[g] = 1 + below(40); }
    const std::vector<uint32_t> off = deform_index_offsets(nt.data(), n_meshes);
    CHECK(off.size() == n_meshes + 1 && off[0] == 0);
    for (size_t g = 0; g < n_meshes; ++g) CHECK(off[g + 1] - off[g] == 3 * nt[g]);
    std::vector<uint32_t> pool(off.back());
    for (size_t g = 0; g < n_meshes; ++g) for (uint32_t k = 0; k < 3 * nt[g]; ++k) pool[off[g] + k] = below(nv[g]);
    const size_t n_inst = 1 + below((uint32_t)(3 * n_meshes));
    std::vector<uint32_t> inst_geom(n_inst);
    for (uint32_t& g : inst_geom) g = below((uint32_t)n_meshes);
    const size_t capacity = deform_staging_capacity(nv.data(), nt.data(), n_meshes);

    for (int round = 0; round < 8; ++round) {
        std::vector<DeformUpdate> ups;
        for (size_t g = 0; g < n_meshes; ++g)
            if (round == 0 || below(2)) ups.push_back(DeformUpdate{(uint32_t)g, nv[g], nt[g], round == 0 || below(2) != 0, round == 0 || below(2) != 0});
        DeformPlan plan;
        CHECK(make_deform_plan(inst_geom.data(), n_inst, nv.data(), nt.data(), n_meshes, off, ups.data(), ups.size(), &plan));
        CHECK(plan.slots.size() == ups.size() && plan.instance_slot.size() == n_inst && plan.moved.size() == n_inst);
        CHECK(plan.staging_floats <= capacity && (round != 0 || plan.staging_floats == capacity));
        size_t at = 0;
        for (size_t k = 0; k < ups.size(); ++k) {
            const DeformSlot& s = plan.slots[k];
            CHECK(s.pos == at); at += 3 * (size_t)ups[k].n_vert;
            if (ups[k].has_nrm) { CHECK(s.nrm == at); at += 3 * (size_t)ups[k].n_vert; } else CHECK(s.nrm == DEFORM_NO_SLOT);
            if (ups[k].has_tangent) { CHECK(s.tangent == at); at += 3 * (size_t)ups[k].n_tri; } else CHECK(s.tangent == DEFORM_NO_SLOT);
            CHECK(s.idx == off[ups[k].geom] && s.n_tri == nt[ups[k].geom] && s.n_vert == nv[ups[k].geom] && s.pad[0] == 0 && s.pad[1] == 0);
        }
        CHECK(at == plan.staging_floats);
        for (size_t i = 0; i < n_inst; ++i) {
            const auto it = std::find_if(ups.begin(), ups.end(), [&](const DeformUpdate& u) { return u.geom == inst_geom[i]; });
            CHECK((plan.moved[i] != 0) == (it != ups.end()));
            CHECK(plan.instance_slot[i] == (it == ups.end() ? DEFORM_NO_SLOT : (uint32_t)(it - ups.begin())));
        }
        // the device's table, and the kernel's gather restated: staging[k] = k, so a gathered value names the float it came from
        const std::vector<uint32_t> table = deform_table(plan);
        const size_t slots_at = deform_table_slots_at(n_inst);
        CHECK(slots_at % 4 == 0 && table.size() == slots_at + ups.size() * DEFORM_SLOT_WORDS);
        for (size_t i = 0; i < slots_at; ++i) CHECK(table[i] == (i < n_inst ? plan.instance_slot[i] : DEFORM_NO_SLOT));
        std::vector<float> staging(plan.staging_floats);
        for (size_t k = 0; k < staging.size(); ++k) staging[k] = (float)k;
        for (size_t i = 0; i < n_inst; ++i) {
            const uint32_t slot = table[i];
            if (slot == DEFORM_NO_SLOT) continue;
            CHECK(slot < ups.size());
            DeformSlot s;
            std::memcpy(&s, table.data() + slots_at + slot * DEFORM_SLOT_WORDS, sizeof(s));
            CHECK(std::memcmp(&s, &plan.slots[slot], sizeof(s)) == 0);
            for (uint32_t t = 0; t < s.n_tri; ++t)
                for (int c = 0; c < 3; ++c) {
                    const uint32_t v = pool[s.idx + 3 * t + c];
                    CHECK(v < s.n_vert);
                    for (int a = 0; a < 3; ++a) {
                        CHECK((size_t)s.pos + 3 * v + a < staging.size() && staging[s.pos + 3 * v + a] == (float)(s.pos + 3 * v + a));
                        if (s.nrm != DEFORM_NO_SLOT) CHECK((size_t)s.nrm + 3 * v + a < staging.size() && s.nrm + 3 * v + a >= s.pos + 3 * s.n_vert);
                    }
                    if (s.tangent != DEFORM_NO_SLOT) CHECK((size_t)s.tangent + 3 * t + c < staging.size());
                }
        }
    }

    // ---- refusals ----
    {
        DeformPlan plan;
        DeformUpdate u{(uint32_t)n_meshes, 3, 1, true, true};
        CHECK(!make_deform_plan(inst_geom.data(), n_inst, nv.data(), nt.data(), n_meshes, off, &u, 1, &plan));            // id out of range
        DeformUpdate two[2] = {{0, nv[0], nt[0], true, false}, {0, nv[0], nt[0], true, false}};
        CHECK(!make_deform_plan(inst_geom.data(), n_inst, nv.data(), nt.data(), n_meshes, off, two, 2, &plan));           // repeated
        if (n_meshes > 1) {
            DeformUpdate rev[2] = {{1, nv[1], nt[1], false, false}, {0, nv[0], nt[0], false, false}};
            CHECK(!make_deform_plan(inst_geom.data(), n_inst, nv.data(), nt.data(), n_meshes, off, rev, 2, &plan));       // descending
        }
        DeformUpdate bad_v{0, nv[0] + 1, nt[0], false, false}, bad_t{0, nv[0], nt[0] + 1, false, false};
        CHECK(!make_deform_plan(inst_geom.data(), n_inst, nv.data(), nt.data(), n_meshes, off, &bad_v, 1, &plan));
        CHECK(!make_deform_plan(inst_geom.data(), n_inst, nv.data(), nt.data(), n_meshes, off, &bad_t, 1, &plan));
        std::vector<uint32_t> short_off(off.begin(), off.end() - 1);
        DeformUpdate ok{0, nv[0], nt[0], false, false};
        CHECK(!make_deform_plan(inst_geom.data(), n_inst, nv.data(), nt.data(), n_meshes, short_off, &ok, 1, &plan));
        std::vector<uint32_t> bad_inst = inst_geom; bad_inst[0] = (uint32_t)n_meshes;
        CHECK(!make_deform_plan(bad_inst.data(), n_inst, nv.data(), nt.data(), n_meshes, off, &ok, 1, &plan));
        CHECK(make_deform_plan(inst_geom.data(), n_inst, nv.data(), nt.data(), n_meshes, off, &ok, 1, &plan));
        CHECK(plan.staging_floats == 3 * (size_t)nv[0] && plan.slots[0].nrm == DEFORM_NO_SLOT && plan.slots[0].tangent == DEFORM_NO_SLOT);
    }
    std::printf("ok %zu\n", n_meshes);
    return 0;
}
