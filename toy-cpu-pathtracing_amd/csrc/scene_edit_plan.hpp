// Editing lights and materials of a built scene (include/mi355pt_edit.h): what the host decides before anything is uploaded, and the table
// reclass_tris_kernel (pt_kernels_edit.hip) reads.  Pure — no HIP header, no environment, no clock, no scene type beyond plain arrays —
// like deform_plan.hpp; tests/scene_edit_plan_check.cpp includes it alone.  Five things live here:
//
//   1. THE CLASS of a material record: the sort key of the deferral queue (pt_kernel.hpp) every triangle record of the material's
//      instances carries.  The lowering (scene_lower.cpp lower_triangles) takes it from here.
//   2. Which materials changed class between two sets of records, and
//   3. the per-material table the device reads: the new class, or EDIT_CLASS_UNCHANGED.
//   4. The reason an edit cannot be done in place (or 0).
//   5. The "same bytes" test of MI355PT_EDIT_SAME_RECORDS.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace pt {

constexpr uint32_t EDIT_CLASS_UNCHANGED = 0xffffffffu;
// the values of layout.hpp the class and the reasons depend on (scene_edit.cpp holds them to the enums)
constexpr uint32_t EDIT_MT_EMISSIVE = 1, EDIT_MT_CLEARCOAT = 4, EDIT_SPK_TEXTURE = 3, EDIT_CLASS_TEXTURED = 8;
// mi355pt_edit_result.reason (include/mi355pt_rebase.h, include/mi355pt_edit.h; scene_edit.cpp holds them to the headers)
constexpr uint32_t EDIT_IN_PLACE = 0, EDIT_UNSUPPORTED_BUILD = 4, EDIT_SAME_RECORDS = 8, EDIT_EMITTER_SET_CHANGED = 9, EDIT_TABLE_SHAPE_CHANGED = 10;

// what of a material record the class and the fallbacks read: DevMaterial::type and the kinds of its three spectra
struct EditMaterialKey { uint32_t type, color_kind, cc_tint_kind, eta_kind; };

// material type, + 8 if the material has a SPECTRUM texture (texel fetches + the rgb2spec lookup: the long branch).  Normal / roughness
// maps alone do not make a class: measured -4 % on scene 5
inline uint32_t edit_material_class(const EditMaterialKey& m) {
    const bool tex = m.color_kind == EDIT_SPK_TEXTURE || m.cc_tint_kind == EDIT_SPK_TEXTURE || m.eta_kind == EDIT_SPK_TEXTURE;
    return m.type | (tex ? EDIT_CLASS_TEXTURED : 0u);
}

// per material: the class of `after` where it differs from the class of `before`, else EDIT_CLASS_UNCHANGED; *n_changed (NULL ok) counts the former
inline std::vector<uint32_t> edit_class_table(const EditMaterialKey* before, const EditMaterialKey* after, size_t n, uint32_t* n_changed = nullptr) {
    std::vector<uint32_t> t(n, EDIT_CLASS_UNCHANGED);
    uint32_t changed = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t c = edit_material_class(after[i]);
        if (c != edit_material_class(before[i])) { t[i] = c; ++changed; }
    }
    if (n_changed) *n_changed = changed;
    return t;
}

inline size_t edit_count_type(const EditMaterialKey* m, size_t n, uint32_t type) {
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) if (m[i].type == type) ++k;
    return k;
}

// EDIT_IN_PLACE, or why the edited description is built again.  A build without the side tables first, as for the other updates; then a
// material that enters or leaves the emitters (the light list, light_tris and the shading records' light index change shape); then the
// number of clearcoat materials (cc_albedo is sized by it)
inline uint32_t edit_fallback_reason(const EditMaterialKey* before, const EditMaterialKey* after, size_t n, bool build_supports_updates) {
    if (!build_supports_updates) return EDIT_UNSUPPORTED_BUILD;
    for (size_t i = 0; i < n; ++i) if ((before[i].type == EDIT_MT_EMISSIVE) != (after[i].type == EDIT_MT_EMISSIVE)) return EDIT_EMITTER_SET_CHANGED;
    if (edit_count_type(before, n, EDIT_MT_CLEARCOAT) != edit_count_type(after, n, EDIT_MT_CLEARCOAT)) return EDIT_TABLE_SHAPE_CHANGED;
    return EDIT_IN_PLACE;
}

// MI355PT_EDIT_SAME_RECORDS: the record array is bytewise the built one.  Bytes, not values: -0.0 is not +0.0, a NaN payload counts
inline bool edit_same_bytes(const void* given, const void* current, size_t bytes) { return bytes == 0 || std::memcmp(given, current, bytes) == 0; }
template <typename T>
inline bool edit_same_bytes(const std::vector<T>& given, const std::vector<T>& current) {
    return given.size() == current.size() && edit_same_bytes(given.data(), current.data(), given.size() * sizeof(T));
}

}  // namespace pt
