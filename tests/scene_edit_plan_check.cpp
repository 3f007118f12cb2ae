// csrc/scene_edit_plan.hpp on its own (tests/test_scene_edit.py builds this with plain g++, and a second time with the host sanitizers):
// the class of every material type with and without a spectrum texture on each of its three spectra, the changed-class table, every
// fallback reason and its order, the same-bytes test on -0.0 / +0.0 and NaN payloads.
//   scene_edit_plan_check <seed> <n materials>      prints "ok ..." and exits 0, or says what is wrong and exits 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "scene_edit_plan.hpp"

using namespace pt;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

int main(int argc, char** argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const size_t n = argc > 2 ? (size_t)std::atoi(argv[2]) : 8u;

    // 1. the class: type | 8 with a spectrum texture on colour, coat tint or eta; no other kind of spectrum makes a class
    for (uint32_t type = 0; type <= 5; ++type) {
        for (uint32_t kind = 0; kind <= 4; ++kind) {
            const uint32_t want = type | (kind == EDIT_SPK_TEXTURE ? 8u : 0u);
            CHECK(edit_material_class(EditMaterialKey{type, kind, 0, 0}) == want);
            CHECK(edit_material_class(EditMaterialKey{type, 0, kind, 0}) == want);
            CHECK(edit_material_class(EditMaterialKey{type, 0, 0, kind}) == want);
        }
        CHECK(edit_material_class(EditMaterialKey{type, 0, 1, 2}) == type);
        CHECK(edit_material_class(EditMaterialKey{type, 3, 3, 3}) == (type | 8u));
    }
    CHECK(edit_material_class(EditMaterialKey{EDIT_MT_EMISSIVE, 2, 0, 0}) == 1u && edit_material_class(EditMaterialKey{EDIT_MT_CLEARCOAT, 3, 0, 0}) == 12u);

    // 2 + 3. the table: the new class exactly where the class differs; a change of anything the class does not read is no entry
    std::mt19937 rng(seed);
    std::vector<EditMaterialKey> before(n), after(n);
    for (size_t i = 0; i < n; ++i) before[i] = EditMaterialKey{(uint32_t)(rng() % 6u), (uint32_t)(rng() % 5u), (uint32_t)(rng() % 5u), (uint32_t)(rng() % 5u)};
    after = before;
    uint32_t n_changed = 77;
    std::vector<uint32_t> t = edit_class_table(before.data(), after.data(), n, &n_changed);
    CHECK(t.size() == n && n_changed == 0);
    for (uint32_t w : t) CHECK(w == EDIT_CLASS_UNCHANGED);
    uint32_t want_changed = 0;
    for (size_t i = 0; i < n; ++i) {
        switch (rng() % 4u) {
            case 0: break;
            case 1: after[i].type = (before[i].type + 1u + rng() % 5u) % 6u; break;                                       // another type: always another class
            case 2: after[i].color_kind = before[i].color_kind == EDIT_SPK_TEXTURE ? 1u : EDIT_SPK_TEXTURE; break;   // the texture bit may flip
            case 3: after[i].eta_kind = before[i].eta_kind == 0u ? 1u : 0u; break;                                        // constant <-> sigmoid: never a class
        }
        if (edit_material_class(before[i]) != edit_material_class(after[i])) ++want_changed;
    }
    t = edit_class_table(before.data(), after.data(), n, &n_changed);
    CHECK(n_changed == want_changed);
    for (size_t i = 0; i < n; ++i) CHECK(t[i] == (edit_material_class(before[i]) != edit_material_class(after[i]) ? edit_material_class(after[i]) : EDIT_CLASS_UNCHANGED));
    CHECK(edit_class_table(before.data(), after.data(), n).size() == n);                                                  // (the count is optional)
    CHECK(edit_class_table(nullptr, nullptr, 0, &n_changed).empty() && n_changed == 0);

    // 4. the reasons, in their order: the build first, then the emitter set, then the clearcoat count
    const EditMaterialKey lambert{0, 1, 0, 0}, emissive{EDIT_MT_EMISSIVE, 2, 0, 0}, glass{2, 0, 0, 0}, coat{EDIT_MT_CLEARCOAT, 1, 1, 0}, coat_tex{EDIT_MT_CLEARCOAT, 3, 1, 0};
    {
        const EditMaterialKey b[3] = {lambert, emissive, coat};
        const EditMaterialKey same[3] = {glass, emissive, coat_tex}, to_emitter[3] = {emissive, emissive, coat}, from_emitter[3] = {lambert, lambert, coat};
        const EditMaterialKey fewer_coats[3] = {lambert, emissive, glass}, more_coats[3] = {coat, emissive, coat}, moved_coat[3] = {coat, emissive, lambert};
        const EditMaterialKey both[3] = {emissive, emissive, glass};
        CHECK(edit_fallback_reason(b, b, 3, true) == EDIT_IN_PLACE && edit_fallback_reason(b, same, 3, true) == EDIT_IN_PLACE);
        CHECK(edit_fallback_reason(b, to_emitter, 3, true) == EDIT_EMITTER_SET_CHANGED && edit_fallback_reason(b, from_emitter, 3, true) == EDIT_EMITTER_SET_CHANGED);
        CHECK(edit_fallback_reason(b, fewer_coats, 3, true) == EDIT_TABLE_SHAPE_CHANGED && edit_fallback_reason(b, more_coats, 3, true) == EDIT_TABLE_SHAPE_CHANGED);
        CHECK(edit_fallback_reason(b, moved_coat, 3, true) == EDIT_IN_PLACE);                                             // the count is what sizes the table
        CHECK(edit_fallback_reason(b, both, 3, true) == EDIT_EMITTER_SET_CHANGED);
        CHECK(edit_fallback_reason(b, b, 3, false) == EDIT_UNSUPPORTED_BUILD && edit_fallback_reason(b, both, 3, false) == EDIT_UNSUPPORTED_BUILD);
        CHECK(edit_fallback_reason(nullptr, nullptr, 0, true) == EDIT_IN_PLACE);
        CHECK(EDIT_IN_PLACE == 0 && EDIT_UNSUPPORTED_BUILD == 4 && EDIT_SAME_RECORDS == 8 && EDIT_EMITTER_SET_CHANGED == 9 && EDIT_TABLE_SHAPE_CHANGED == 10);
    }

    // 5. same bytes: bytes, not values
    {
        const float pz[2] = {0.0f, 1.0f}, nz[2] = {-0.0f, 1.0f};
        CHECK(pz[0] == nz[0] && !edit_same_bytes(pz, nz, sizeof(pz)) && edit_same_bytes(pz, pz, sizeof(pz)));
        const uint32_t nan_a = 0x7fc00001u, nan_b = 0x7fc00002u;
        float a, b, a2;
        std::memcpy(&a, &nan_a, 4); std::memcpy(&b, &nan_b, 4); std::memcpy(&a2, &nan_a, 4);
        CHECK(std::isnan(a) && std::isnan(b) && a != a2 && edit_same_bytes(&a, &a2, 4) && !edit_same_bytes(&a, &b, 4));
        CHECK(edit_same_bytes(nullptr, nullptr, 0));
        const std::vector<float> v1{1.0f, 2.0f}, v2{1.0f, 2.0f}, v3{1.0f}, v4{1.0f, -2.0f}, none;
        CHECK(edit_same_bytes(v1, v2) && !edit_same_bytes(v1, v3) && !edit_same_bytes(v1, v4) && edit_same_bytes(none, none));
    }
    std::printf("ok seed=%u materials=%zu changed=%u\n", seed, n, want_changed);
    return 0;
}
