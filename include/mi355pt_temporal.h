/*
 * mi355pt_temporal.h — the temporal-reprojection block of the C ABI (included by mi355pt.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart: the TEMPORAL half of the SVGF (Schied et al., HPG 2017) that mi355pt_denoise_var.h cites, and the
 * consumer of the position and hit films of mi355pt_gbuffer.h.  Each pixel of the current frame is reprojected into the previous camera's
 * image through its hit position; the previous frame's ACCUMULATED film is gathered there with a bilinear footprint whose taps are tested
 * against the current surface (plane distance, shading normal), and the current frame is blended in with the weight 1 / history length.
 * A few spp per frame then converge over the frames of a camera move instead of starting from zero each frame.  Only the camera moves.
 *
 * The text below is normative: tests/temporal_reference.py restates it in NumPy.  All arithmetic is binary32, every operation rounded on
 * its own (no fused multiply-add, no transcendental function, IEEE division), no atomics and a fixed summation order: two runs are
 * bit-equal, and the device result is bit-equal to the restatement.
 *
 * Buffers are row-major, y down.  A frame (mi355pt_temporal_frame) holds W x H x 3 f32 films and one W x H f32 length film:
 *   the CURRENT frame   film = beauty SUMS B of `spp` samples, half = the half-film SUMS H of its first spp / 2 (NULL: no half film),
 *                       length ignored; position, shading_normal, hit = the raw G-buffer SUMS of mi355pt_gbuffer.h (any sample count).
 *   the PREVIOUS frame  film, half, length = what this call wrote for that frame (out_film, out_half, out_length); position,
 *                       shading_normal, hit = that frame's raw G-buffer sums.
 * A view (mi355pt_temporal_view) says how a render-space point of the current frame lands in the previous frame's image.
 *
 * Per pixel p = (x, y):
 *   Current values.  With a half film:  c1 = clean(H / (spp / 2)),  c2 = clean((B - H) / (spp / 2))  per channel; without:  c = clean(B / spp).
 *     clean is the rule of mi355pt_denoise_var.h: a non-finite or negative value becomes 0.  Everything below that is said of c and m holds
 *     for c1, m1 and for c2, m2 alike.
 *   Geometry.  h = hit.y;  X = position / h per component;  nrm = 2 (shading_normal / h) - 1 per component, NOT renormalised;
 *     t = hit.x / h.  h == 0: no history.
 *   Projection.  Xp = X + delta;  v_i = ((rows[3i] Xp.x + rows[3i+1] Xp.y) + rows[3i+2] Xp.z), i = 0, 1, 2;  zc = -v_2.
 *     !(zc > 0): no history.   fx = cx + (v_0 / zc) sx;  fy = cy - (v_1 / zc) sy;  gx = fx - 0.5;  gy = fy - 0.5.
 *     !(gx >= -1 && gx < W && gy >= -1 && gy < H) (W, H as binary32; a NaN fails): no history.
 *     x0 = floor(gx), wx = gx - x0;  y0 = floor(gy), wy = gy - y0.
 *   Taps.  q_0 .. q_3 = (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with the bilinear weights b_0 .. b_3 = (1-wx)(1-wy), wx (1-wy),
 *     (1-wx) wy, wx wy.  A tap q is VALID iff it lies in the frame and, with hq = hit_prev.y[q]:
 *         hq > 0;   length_prev[q] > 0;
 *         |((e.x nrm.x + e.y nrm.y) + e.z nrm.z)| <= pos_tol t,   e = Xp - position_prev[q] / hq
 *             (the distance from the current surface's PLANE in units of the hit distance: a grazing surface keeps its history);
 *         ((nrm.x nq.x + nrm.y nq.y) + nrm.z nq.z) >= normal_cos,   nq = 2 (shading_normal_prev[q] / hq) - 1.
 *     (A NaN fails either comparison.)  A valid tap has the weight w_k = b_k and its film values; an invalid tap has the weight 0 AND the
 *     film values 0, whatever the buffers hold there.   Wt = ((w_0 + w_1) + w_2) + w_3.
 *   With history (none of the "no history" cases, and Wt > min_weight), per channel and in the order of Wt:
 *         with a half film    hist1 = (sum_k w_k half_prev[q_k]) / Wt,    hist2 = (sum_k w_k (film_prev[q_k] - half_prev[q_k])) / Wt
 *         without             hist  = (sum_k w_k film_prev[q_k]) / Wt
 *         Lh = (sum_k w_k length_prev[q_k]) / Wt;   L = min(Lh + 1, max_history);   a = 1 / L;   m = hist + (c - hist) a.
 *   Without history:  m = c,  L = 1.   Without a previous frame every pixel is without history, and the G-buffer films are not read.
 *   Outputs.  out_length = L.   With a half film  out_half = m1,  out_film = m1 + m2: a film pair with spp = 2 in the convention "F = all,
 *     H = first half", which mi355pt_denoise_var_device(out_film, out_half, 2, ...) and mi355pt_film_resolve_device(out_film, .., 2, ..)
 *     take as it is.  Without  out_film = m: a linear MEAN, spp = 1.   Every pixel of every output is written.
 *
 * B and H of the current frame may hold anything (cleaned as above).  The previous film and half film must be FINITE where the previous
 * length is > 0 (what this call wrote is); elsewhere every buffer may hold anything.
 */
#ifndef MI355PT_TEMPORAL_H
#define MI355PT_TEMPORAL_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* plain data: how a render-space point of the CURRENT frame lands in the PREVIOUS frame's image */
typedef struct mi355pt_temporal_view {
    float delta[3];       /* cur.position - prev.position: X_prev = X_cur + delta (render space = world - camera position) */
    float rows[9];        /* world -> previous camera space: the rows s, u, -f of look_to_rh(prev.direction, prev.up) (camera.rs:61 is its transpose) */
    float sx, sy, cx, cy; /* sx = (W/2) / (aspect tan(fov/2)), sy = (H/2) / tan(fov/2), cx = W/2, cy = H/2 (the inverse of camera.rs:53-58) */
} mi355pt_temporal_view;

typedef struct mi355pt_temporal_params {
    float pos_tol, normal_cos, min_weight, max_history;
} mi355pt_temporal_params;

/* device pointers for the _device entry point, host pointers for mi355pt_temporal_accumulate */
typedef struct mi355pt_temporal_frame {
    const float *film, *half, *length;            /* current: beauty sums, half-film sums (NULL ok), ignored; previous: the accumulated pair and its length */
    const float *position, *shading_normal, *hit; /* the frame's raw G-buffer sums (mi355pt_gbuffer.h), required */
} mi355pt_temporal_frame;

/* pos_tol 0.01, normal_cos 0.9, min_weight 0.01, max_history 32 */
void mi355pt_temporal_params_default(mi355pt_temporal_params* out);
/* The view of a camera pair.  Host only, no device needed.  Computed in double from the f32 fields, each entry rounded once to f32;
 * direction and up are normalised as set_look_to does (camera.rs:39-48).  Returns MI355PT_E_INVALID for a NULL pointer, differing or zero
 * width / height, differing fov_deg, a zero (or non-finite) direction or up, or a direction parallel to up. */
int mi355pt_temporal_view_from_cameras(const mi355pt_camera* cur, const mi355pt_camera* prev, mi355pt_temporal_view* out);
/* The accumulation on device buffers: ONE launch.  Asynchronous on `hip_stream` (a hipStream_t, NULL = default stream); allocates nothing,
 * synchronises nothing.  prev == NULL (then view must be NULL too) is the first frame.  d_out_half is NULL iff cur->half is NULL.
 * Returns MI355PT_E_INVALID — before anything touches the device — when: cur, params, d_out_film, d_out_length, or a required film of a
 * given frame is NULL (film, position, shading_normal, hit; length of prev); prev and view are not both NULL or both given; the half
 * pointers of cur, prev (when given) and the output are not all NULL or all given; spp is 0, or odd with a half film; width or height is
 * 0 (or above 2^24, or the frame has more than 2^31 - 1 blocks of 64 x 4 pixels); pos_tol, min_weight or max_history is not finite or not > 0;
 * max_history < 1; normal_cos is not in [-1, 1] (a zero-initialised params struct is refused, never interpreted); an output pointer
 * equals an input pointer (cur->length, which is ignored, aside) or another output. */
int mi355pt_temporal_accumulate_device(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                       const mi355pt_temporal_view* view, uint32_t width, uint32_t height,
                                       const mi355pt_temporal_params* params, float* d_out_film, float* d_out_half, float* d_out_length,
                                       void* hip_stream);
/* The same with host buffers: allocates the device buffers, copies, runs mi355pt_temporal_accumulate_device on the default stream,
 * synchronises and copies the outputs back.  Same argument checks, before any allocation. */
int mi355pt_temporal_accumulate(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* params,
                                float* out_film, float* out_half, float* out_length);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_TEMPORAL_H */
