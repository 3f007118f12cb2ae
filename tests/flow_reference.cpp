// TEST INFRASTRUCTURE ONLY: the CPU side of the flow pass's hit check (include/mi355pt_flow.h) on top of the oracle's own Camera and
// Scene::intersect.  One translation unit that includes the oracle's C API, like tests/ids_reference.cpp, so the library built from it
// carries the oracle's scene-construction functions under the same `ptoracle_` prefix.  It shares no code with the HIP kernel
// (csrc/pt_kernels_flow.hip).
#include "oracle_api.cpp"

extern "C" {

// Per pixel of the 8x8 tiles of the shard in `p`, for the ray through the pixel CENTRE — camera.sample_ray(p, (0.5, 0.5)), not moved
// forward —: hits[2 i] = the primitive (= instance) index + 1 of the closest hit, or 0 for a miss; hits[2 i + 1] = the triangle's index
// inside its mesh; pos[3 i ..] = the hit's render-space position (the interaction's).  Pixels outside the shard are not written.
// -1 for a null buffer or a zero-sized frame.
int ptoracle_render_flow_hits(ptoracle_scene* s, const mi355pt_camera* c, const mi355pt_params* p, uint32_t* hits, float* pos) {
    if (!hits || !pos || c->width == 0 || c->height == 0) return -1;
    const Camera cam = make_camera(c);
    const uint32_t W = c->width, H = c->height, tiles_x = (W + 7) / 8;
    const uint32_t sc = p->shard_count ? p->shard_count : 1, si = p->shard_count ? p->shard_index : 0;
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            if (((y / 8) * tiles_x + (x / 8)) % sc != si) continue;
            const Ray ray = cam.sample_ray(x, y, V2{0.5f, 0.5f});
            Intersection hit;
            const bool got = s->scene.intersect(ray, std::numeric_limits<float>::max(), &hit, nullptr);
            const size_t i = (size_t)y * W + x;
            hits[2 * i] = got ? (uint32_t)hit.primitive + 1u : 0u;
            hits[2 * i + 1] = got ? hit.triangle : 0u;
            pos[3 * i] = got ? hit.interaction.position.x : 0.0f;
            pos[3 * i + 1] = got ? hit.interaction.position.y : 0.0f;
            pos[3 * i + 2] = got ? hit.interaction.position.z : 0.0f;
        }
    return 0;
}

}  // extern "C"
