// Deforming meshes of a built scene (include/mi355pt_deform.h): what the host lays out for deform_tris_kernel (pt_kernels_deform.hip).
// Pure — no HIP header, no environment, no clock, no scene type beyond plain arrays — like instance_move_plan.hpp;
// tests/deform_plan_check.cpp includes it alone.  Three things live here:
//
//   1. THE LAYOUT of one call: the new arrays of all updated meshes in ONE staging buffer of floats (per mesh: positions, then the normals
//      and the tangents where given), one DeformSlot per updated mesh naming its offsets, and per instance the slot of its mesh or
//      DEFORM_NO_SLOT.  The index buffers of all meshes of a scene live in one pool of words, mesh after mesh (deform_index_offsets).
//   2. The moved mask: every instance of an updated mesh (what lower_camera_records and shade_refresh_kernel take).
//   3. The "same bytes" test of MI355PT_MOVE_SAME_VERTICES.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace pt {

constexpr uint32_t DEFORM_NO_SLOT = 0xffffffffu;      // an instance whose mesh is not updated; an array that is not given
constexpr uint32_t DEFORM_SLOT_WORDS = 8;

// one updated mesh as the device sees it: offsets in floats into the staging buffer, in words into the index pool.  32 bytes: two 16-byte loads
struct DeformSlot {
    uint32_t pos;           // n_vert x 3 floats
    uint32_t nrm;           // n_vert x 3 floats, or DEFORM_NO_SLOT: the normals stay
    uint32_t tangent;       // n_tri x 3 floats, or DEFORM_NO_SLOT: the tangents stay
    uint32_t idx;           // n_tri x 3 words of the index pool
    uint32_t n_tri, n_vert; // the kernel's bounds: a triangle or an index past them is not followed
    uint32_t pad[2];
};
static_assert(sizeof(DeformSlot) == DEFORM_SLOT_WORDS * 4, "slot record");

// one update as the plan takes it
struct DeformUpdate {
    uint32_t geom, n_vert, n_tri;
    bool has_nrm, has_tangent;
};

struct DeformPlan {
    std::vector<DeformSlot> slots;          // one per update, in the updates' order
    std::vector<uint32_t> instance_slot;    // per instance: index into slots, or DEFORM_NO_SLOT
    std::vector<uint8_t> moved;             // per instance: 1 = its mesh is updated
    size_t staging_floats = 0;
};

// first word of each mesh's indices in the pool, and the pool's size as the last entry (n_meshes + 1 entries)
inline std::vector<uint32_t> deform_index_offsets(const uint32_t* mesh_n_tri, size_t n_meshes) {
    std::vector<uint32_t> off(n_meshes + 1, 0u);
    for (size_t g = 0; g < n_meshes; ++g) off[g + 1] = off[g] + 3u * mesh_n_tri[g];
    return off;
}
// the largest staging buffer a call on this scene can need: every mesh updated with all three arrays
inline size_t deform_staging_capacity(const uint32_t* mesh_n_vert, const uint32_t* mesh_n_tri, size_t n_meshes) {
    size_t n = 0;
    for (size_t g = 0; g < n_meshes; ++g) n += (size_t)6 * mesh_n_vert[g] + (size_t)3 * mesh_n_tri[g];
    return n;
}

// false: a geom id out of range, ids not strictly ascending, counts that differ from the mesh's, or offsets that do not fit 32 bits
inline bool make_deform_plan(const uint32_t* instance_geom, size_t n_instances, const uint32_t* mesh_n_vert, const uint32_t* mesh_n_tri, size_t n_meshes,
                             const std::vector<uint32_t>& index_offsets, const DeformUpdate* updates, size_t n_updates, DeformPlan* out) {
    *out = DeformPlan{};
    if (index_offsets.size() != n_meshes + 1) return false;
    std::vector<uint32_t> slot_of_mesh(n_meshes, DEFORM_NO_SLOT);
    size_t at = 0;
    for (size_t k = 0; k < n_updates; ++k) {
        const DeformUpdate& u = updates[k];
        if (u.geom >= n_meshes || (k && u.geom <= updates[k - 1].geom)) return false;
        if (u.n_vert != mesh_n_vert[u.geom] || u.n_tri != mesh_n_tri[u.geom]) return false;
        DeformSlot s{};
        s.pos = (uint32_t)at; at += (size_t)3 * u.n_vert;
        s.nrm = DEFORM_NO_SLOT; s.tangent = DEFORM_NO_SLOT;
        if (u.has_nrm) { s.nrm = (uint32_t)at; at += (size_t)3 * u.n_vert; }
        if (u.has_tangent) { s.tangent = (uint32_t)at; at += (size_t)3 * u.n_tri; }
        if (at >= (size_t)DEFORM_NO_SLOT) return false;
        s.idx = index_offsets[u.geom];
        s.n_tri = u.n_tri; s.n_vert = u.n_vert;
        slot_of_mesh[u.geom] = (uint32_t)out->slots.size();
        out->slots.push_back(s);
    }
    out->staging_floats = at;
    out->instance_slot.assign(n_instances, DEFORM_NO_SLOT);
    out->moved.assign(n_instances, 0);
    for (size_t i = 0; i < n_instances; ++i) {
        if (instance_geom[i] >= n_meshes) return false;
        out->instance_slot[i] = slot_of_mesh[instance_geom[i]];
        out->moved[i] = out->instance_slot[i] != DEFORM_NO_SLOT ? 1 : 0;
    }
    return true;
}

// the table the device reads: n_instances words (the slot per instance), then DEFORM_SLOT_WORDS words per slot, the slots starting at a
// multiple of 4 words so that a slot record is two aligned 16-byte loads
inline size_t deform_table_slots_at(size_t n_instances) { return (n_instances + 3u) & ~(size_t)3u; }
inline std::vector<uint32_t> deform_table(const DeformPlan& plan) {
    const size_t at = deform_table_slots_at(plan.instance_slot.size());
    std::vector<uint32_t> t(at + plan.slots.size() * DEFORM_SLOT_WORDS, DEFORM_NO_SLOT);
    if (!plan.instance_slot.empty()) std::memcpy(t.data(), plan.instance_slot.data(), plan.instance_slot.size() * sizeof(uint32_t));
    if (!plan.slots.empty()) std::memcpy(t.data() + at, plan.slots.data(), plan.slots.size() * sizeof(DeformSlot));
    return t;
}

// MI355PT_MOVE_SAME_VERTICES: the given array is bytewise the current one (a null `given` = keep = the same).  Bytes, not values: -0.0
// is not +0.0, a NaN payload counts
inline bool deform_same_bytes(const float* given, const float* current, size_t n_floats) {
    return !given || n_floats == 0 || std::memcmp(given, current, n_floats * sizeof(float)) == 0;
}

}  // namespace pt
