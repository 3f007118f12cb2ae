// The gather of the temporal reprojection (include/mi355pt_temporal.h) as the BODY of a kernel, included by the two kernels that run it —
// the way pt_kernel_body.inc is the body of pt_kernel and of pt_kernel_tiles.  The including kernel is a template on <bool HAS_HALF,
// bool HAS_PREV> with the parameters (TemporalFrameDev cur, TemporalFrameDev prev, TemporalArgs a), runs one thread per pixel on the grid of
// denoise_grid_blocks with DN_BLOCK_X x DN_BLOCK_Y blocks, and defines the EPILOGUE before the #include:
//   PT_TP_RECORD == false   the blend of mi355pt_temporal.h.  After the body:  p (the pixel), m1[3], m2[3] (m, 0 without a half film), L.
//   PT_TP_RECORD == true    no blend (the current film is then not read at all: c1, c2 are dead).  After the body:  p, and the gathered
//                           history m1 = hist1, m2 = hist2 (hist, 0 without a half film), L = min(Lh + 1, max_history), or L = 0 and
//                           m1 = m2 = 0 for a pixel without history.
// A thread outside the frame has returned.
//   PT_TP_MOTION == false   the static world of mi355pt_temporal.h: Xp = X + a.delta.  The text of the kernels as they were.
//   PT_TP_MOTION == true    include/mi355pt_motion.h: the including kernel has one more template parameter, bool HAS_PREV_IDS, and one
//                           more kernel parameter, MotionArgs mo.  The pixel's id picks a record of mo.table, which carries X and nrm
//                           into the previous render space (a.delta is not read); with HAS_PREV_IDS a tap must show the pixel's id.
//   PT_TP_MOTION == 2       include/mi355pt_flow.h: the template parameters of PT_TP_MOTION == true, and FlowArgs fl in the place of mo.
//                           The pixel's own record of fl.flow is ADDED to X and to nrm (a.delta is not read); with HAS_PREV_IDS a tap
//                           must show fl.ids_cur[p], which is not read otherwise.
//
// A pixel's hit position is projected into the previous camera, and the previous frame's accumulated films are gathered with a 2 x 2
// bilinear footprint.  The four taps' loads are UNCONDITIONAL, at indices clamped to the frame: whether a pixel has a history at all (no
// hit, behind the previous camera, outside its image) and whether a tap is valid (in frame, hit, plane distance, normal) are selects on the
// loaded values, never branches around loads — as the 3 x 3 of pt_kernels_denoise_var.hip.  All gathers of a pixel are in flight together.
// Neighbouring lanes reproject to neighbouring texels, so the gathers are served by L1 / L2.  (What the compiler does form is a skip around
// the blend's divisions for a wave in which no pixel has a history: arithmetic only, after every load.)
    const uint32_t bx = blockIdx.x % a.blocks_x, by = blockIdx.x / a.blocks_x;
    const uint32_t x = bx * DN_BLOCK_X + threadIdx.x, y = by * DN_BLOCK_Y + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;

    // the current values
    const float3u B = tp_load3(cur.film, p);
    float c1[3], c2[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (HAS_HALF) {
        const float3u H = tp_load3(cur.half, p);
        c1[0] = dn_clean(H.x, a.half_spp); c1[1] = dn_clean(H.y, a.half_spp); c1[2] = dn_clean(H.z, a.half_spp);
        c2[0] = dn_clean(B.x - H.x, a.half_spp); c2[1] = dn_clean(B.y - H.y, a.half_spp); c2[2] = dn_clean(B.z - H.z, a.half_spp);
    } else {
        c1[0] = dn_clean(B.x, a.spp); c1[1] = dn_clean(B.y, a.spp); c1[2] = dn_clean(B.z, a.spp);
    }
    float m1[3] = {c1[0], c1[1], c1[2]}, m2[3] = {c2[0], c2[1], c2[2]}, L = 1.0f;
    if constexpr (PT_TP_RECORD) {
        m1[0] = m1[1] = m1[2] = 0.0f; m2[0] = m2[1] = m2[2] = 0.0f; L = 0.0f;
    }

    if constexpr (HAS_PREV) {
        // geometry of p (h == 0 makes NaNs and infinities: `ok` selects them away)
#if PT_TP_MOTION == 2
        // the pixel's motion record (two 16-byte loads, coalesced) and, for the id test, its id — issued ahead of the geometry's divisions
        const float4* const frec = (const float4*)(fl.flow + p);
        const float4 fr0 = frec[0], fr1 = frec[1];
        uint32_t idc = 0u;
        if constexpr (HAS_PREV_IDS) idc = fl.ids_cur[p];
#elif PT_TP_MOTION
        // the pixel's id and its motion record (six 16-byte loads), issued ahead of the geometry's divisions: one dependent round trip
        // more than the static kernel has, and it is over when the quotients are
        const uint32_t idc = mo.ids_cur[p];
        const float4* const mrec = (const float4*)(mo.table + (idc < mo.last_entry ? idc : mo.last_entry));
        const float4 m0 = mrec[0], m1r = mrec[1], m2r = mrec[2], m3 = mrec[3], m4 = mrec[4], m5 = mrec[5];
#endif
        const float3u P = tp_load3(cur.position, p), N = tp_load3(cur.shading_normal, p);
        const float hx = cur.hit[3 * p], h = cur.hit[3 * p + 1];
#if PT_TP_MOTION == 2
        const float Xx = P.x / h + fr0.x, Xy = P.y / h + fr0.y, Xz = P.z / h + fr0.z;                      // Xp = X + d
        const float nx = (2.0f * (N.x / h) - 1.0f) + fr1.x, ny = (2.0f * (N.y / h) - 1.0f) + fr1.y, nz = (2.0f * (N.z / h) - 1.0f) + fr1.z;
#elif PT_TP_MOTION
        // a = m0.xyzw m1r.xyzw m2r.x,  b = m2r.yzw,  n = m3.xyzw m4.xyzw m5.x: Xp = a X + b, nrm = n nrm — both in the previous render space
        const float X0 = P.x / h, X1 = P.y / h, X2 = P.z / h;
        const float Xx = tp_dot(m0.x, m0.y, m0.z, X0, X1, X2) + m2r.y, Xy = tp_dot(m0.w, m1r.x, m1r.y, X0, X1, X2) + m2r.z,
                    Xz = tp_dot(m1r.z, m1r.w, m2r.x, X0, X1, X2) + m2r.w;
        const float n0 = 2.0f * (N.x / h) - 1.0f, n1 = 2.0f * (N.y / h) - 1.0f, n2 = 2.0f * (N.z / h) - 1.0f;
        const float nx = tp_dot(m3.x, m3.y, m3.z, n0, n1, n2), ny = tp_dot(m3.w, m4.x, m4.y, n0, n1, n2), nz = tp_dot(m4.z, m4.w, m5.x, n0, n1, n2);
#else
        const float Xx = P.x / h + a.delta[0], Xy = P.y / h + a.delta[1], Xz = P.z / h + a.delta[2];        // Xp
        const float nx = 2.0f * (N.x / h) - 1.0f, ny = 2.0f * (N.y / h) - 1.0f, nz = 2.0f * (N.z / h) - 1.0f;
#endif
        const float t = hx / h;
        // projection into the previous image
        const float vx = tp_dot(a.rows[0], a.rows[1], a.rows[2], Xx, Xy, Xz);
        const float vy = tp_dot(a.rows[3], a.rows[4], a.rows[5], Xx, Xy, Xz);
        const float zc = -tp_dot(a.rows[6], a.rows[7], a.rows[8], Xx, Xy, Xz);
        const float gx = (a.cx + (vx / zc) * a.sx) - 0.5f, gy = (a.cy - (vy / zc) * a.sy) - 0.5f;
        const bool ok = h != 0.0f && zc > 0.0f && gx >= -1.0f && gx < a.wf && gy >= -1.0f && gy < a.hf;
        const float gxs = ok ? gx : 0.0f, gys = ok ? gy : 0.0f;           // (a finite value in [-1, W): the conversions below are defined)
        const float x0f = floorf(gxs), y0f = floorf(gys);
        const float wx = gxs - x0f, wy = gys - y0f;
        const int x0 = (int)x0f, y0 = (int)y0f;                           // -1 .. W - 1, -1 .. H - 1
        const float omx = 1.0f - wx, omy = 1.0f - wy;
        const float bw[4] = {omx * omy, wx * omy, omx * wy, wx * wy};
        const float tol = a.pos_tol * t;
        const int wm1 = (int)a.width - 1, hm1 = (int)a.height - 1;

        // the four taps: every load at an index clamped to the frame, issued whatever `ok` and the tap's validity are
        float w[4], len[4], hq[4];
        bool inside[4];
        float3u Pq[4], Nq[4], f[4], g[4];
#if PT_TP_MOTION
        bool same[4] = {true, true, true, true};          // the tap shows the pixel's instance (always, without the previous frame's ids)
#endif
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
            inside[k] = qx >= 0 && qx <= wm1 && qy >= 0 && qy <= hm1;
            const int cx = qx < 0 ? 0 : (qx > wm1 ? wm1 : qx), cy = qy < 0 ? 0 : (qy > hm1 ? hm1 : qy);
            const size_t q = (size_t)cy * a.width + (size_t)cx;
            hq[k] = prev.hit[3 * q + 1];
            len[k] = prev.length[q];
            Pq[k] = tp_load3(prev.position, q); Nq[k] = tp_load3(prev.shading_normal, q);
            f[k] = tp_load3(prev.film, q);
            if constexpr (HAS_HALF) g[k] = tp_load3(prev.half, q);
#if PT_TP_MOTION == 2
            if constexpr (HAS_PREV_IDS) same[k] = fl.ids_prev[q] == idc;
#elif PT_TP_MOTION
            if constexpr (HAS_PREV_IDS) same[k] = mo.ids_prev[q] == idc;
#endif
        }
        // The film values are needed only where the tap turns out valid, and the compiler would sink their loads into a branch on that
        // (it turns a select whose operand is a load into control flow): the gathers would wait for the geometry loads and the arithmetic on
        // them, one tap after the other.  tp_keep pins the loaded values here, after all four taps' loads have been issued
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tp_keep(f[k]);
            if constexpr (HAS_HALF) tp_keep(g[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float ex = Xx - Pq[k].x / hq[k], ey = Xy - Pq[k].y / hq[k], ez = Xz - Pq[k].z / hq[k];
            const float pd = fabsf(tp_dot(ex, ey, ez, nx, ny, nz));
            const float qnx = 2.0f * (Nq[k].x / hq[k]) - 1.0f, qny = 2.0f * (Nq[k].y / hq[k]) - 1.0f, qnz = 2.0f * (Nq[k].z / hq[k]) - 1.0f;
            const float nd = tp_dot(nx, ny, nz, qnx, qny, qnz);
#if PT_TP_MOTION
            const bool valid = ok && inside[k] && hq[k] > 0.0f && len[k] > 0.0f && pd <= tol && nd >= a.normal_cos && same[k];
#else
            const bool valid = ok && inside[k] && hq[k] > 0.0f && len[k] > 0.0f && pd <= tol && nd >= a.normal_cos;
#endif
            w[k] = valid ? bw[k] : 0.0f;
            len[k] = valid ? len[k] : 0.0f;
            f[k] = float3u{valid ? f[k].x : 0.0f, valid ? f[k].y : 0.0f, valid ? f[k].z : 0.0f};
            if constexpr (HAS_HALF) g[k] = float3u{valid ? g[k].x : 0.0f, valid ? g[k].y : 0.0f, valid ? g[k].z : 0.0f};
        }
        const float Wt = ((w[0] + w[1]) + w[2]) + w[3];
        const bool has = Wt > a.min_weight;
        const float Lh = (((w[0] * len[0] + w[1] * len[1]) + w[2] * len[2]) + w[3] * len[3]) / Wt;
        const float Lc = fminf(Lh + 1.0f, a.max_history);
        const float alpha = 1.0f / Lc;
        if constexpr (PT_TP_RECORD) L = has ? Lc : 0.0f;
        else L = has ? Lc : 1.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float fv[4], gv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                fv[k] = ch == 0 ? f[k].x : (ch == 1 ? f[k].y : f[k].z);
                if constexpr (HAS_HALF) gv[k] = ch == 0 ? g[k].x : (ch == 1 ? g[k].y : g[k].z);
            }
            if constexpr (HAS_HALF) {
                const float hist1 = (((w[0] * gv[0] + w[1] * gv[1]) + w[2] * gv[2]) + w[3] * gv[3]) / Wt;
                const float hist2 = (((w[0] * (fv[0] - gv[0]) + w[1] * (fv[1] - gv[1])) + w[2] * (fv[2] - gv[2])) + w[3] * (fv[3] - gv[3])) / Wt;
                if constexpr (PT_TP_RECORD) {
                    m1[ch] = has ? hist1 : 0.0f;
                    m2[ch] = has ? hist2 : 0.0f;
                } else {
                    const float b1 = hist1 + (c1[ch] - hist1) * alpha, b2 = hist2 + (c2[ch] - hist2) * alpha;
                    m1[ch] = has ? b1 : c1[ch];
                    m2[ch] = has ? b2 : c2[ch];
                }
            } else {
                const float hist = (((w[0] * fv[0] + w[1] * fv[1]) + w[2] * fv[2]) + w[3] * fv[3]) / Wt;
                if constexpr (PT_TP_RECORD) {
                    m1[ch] = has ? hist : 0.0f;
                } else {
                    const float b1 = hist + (c1[ch] - hist) * alpha;
                    m1[ch] = has ? b1 : c1[ch];
                }
            }
        }
    }
