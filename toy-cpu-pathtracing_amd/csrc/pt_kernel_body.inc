// The body of the sample-loop kernel: the text between the braces of pt_kernel (pt_kernel.hpp) and of pt_kernel_tiles (pt_kernel_tiles.hpp),
// which differ in ONE thing, how a work item finds its 8x8 tile — PT_LANE_JOB names the function (lane_job: the shard's arithmetic
// progression; lane_job_tiles: an explicit list).  Included, not called: even a helper called from pt_kernel changes the schedule of every
// tuned kernel, and those are measured as they are (tools/asm_identity.sh compares the device assembly with a revision's).
// Expects the kernel's parameters (sc, cam, prm_in, dim_hash_tab, accum, partial, work_counter, stats, pout, defer_buf) and STATS, FEAT, MODE.
    __shared__ __attribute__((aligned(16))) uint32_t s_stack[STACK_DEPTH * 64];    // (16 B: between two traversals it stages tail-queue records as float4, below)
#ifndef PT_FILM_PIX
#define PT_FILM_PIX 64
#endif
    __shared__ float s_film[PT_FILM_PIX * 3];                 // the work item's 8x8 film tile
    __shared__ uint32_t s_hi[SOBOL_HI_DIMS];
    __shared__ uint32_t s_p6[SOBOL_HI_DIMS];
    __shared__ unsigned s_work;
    // The clearcoat kernels run 12 waves per CU, so each has 3.4 KB of LDS the 16-wave kernels do not: the record of the BSDF sample that
    // spawned the ray in flight (f, pdf, the vertex left: 8 dwords per lane, read only at the start of the next vertex's shading) waits there
    // during the traversals instead of in registers the allocator would spill to scratch
    constexpr bool PARK = (FEAT & FEAT_CC) != 0u && kernel_min_waves<FEAT>() <= 3;
    __shared__ float s_park[PARK ? 8 * 64 : 1];
    __shared__ uint8_t s_perm[96];
    __shared__ uint32_t s_ring[ANY_RING];
    __shared__ uint32_t s_occl[2];
    __shared__ uint32_t s_pair[64];
    const AnyLds any_lds{s_ring, s_occl, s_pair};
    __shared__ unsigned long long s_best[64];
    const ClosestLds closest_lds{s_ring, s_best, s_pair};
    __shared__ uint32_t s_infl[2];
    const PairLds pair_lds{s_ring, s_best, s_occl, s_pair, s_infl};
    constexpr bool CAMLIST = !STATS && tail_queue<FEAT, MODE>();          // camera rays from the work item's candidate list (pt_kernel.hpp)
    __shared__ uint32_t s_cand[CAMLIST ? CAM_LIST_CAP : 1u];
    DevParams prm = prm_in;
    if constexpr (MODE == MODE_MIS_SOBOL) { prm.strategy = 2u; prm.sampler = 1u; }
    if constexpr (MODE == MODE_NEE_SOBOL) { prm.strategy = 1u; prm.sampler = 1u; }
    if constexpr (MODE == MODE_PT) prm.strategy = 0u;                      // either sampler
    const uint32_t lane = threadIdx.x;
    auto park = [&](Path& Q, bool mine = true) {      // `mine`: this lane's record is stored (a second shading pass only stores the lanes it shaded)
        if constexpr (PARK) {
            if (mine) {
#pragma unroll
                for (int i = 0; i < 4; ++i) s_park[i * 64 + lane] = Q.pf[i];
                s_park[4 * 64 + lane] = Q.p_pdf; s_park[5 * 64 + lane] = Q.prev_pos.x; s_park[6 * 64 + lane] = Q.prev_pos.y; s_park[7 * 64 + lane] = Q.prev_pos.z;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) Q.pf[i] = 0.0f;
            Q.p_pdf = 0.0f; Q.prev_pos = mk3(0.0f, 0.0f, 0.0f);
        }
    };
    auto unpark = [&](Path& Q) {
        if constexpr (PARK) {
#pragma unroll
            for (int i = 0; i < 4; ++i) Q.pf[i] = s_park[i * 64 + lane];
            Q.p_pdf = s_park[4 * 64 + lane]; Q.prev_pos = mk3(s_park[5 * 64 + lane], s_park[6 * 64 + lane], s_park[7 * 64 + lane]);
        }
    };
    uint32_t* stack = s_stack + lane;
    // murmur(dimension, seed) comes straight from its 1 KB global table (L1-resident): the LDS it used holds the tile's film
    for (uint32_t k = lane; k < 96u; k += 64u) s_perm[k] = (uint8_t)((perm_packed(k >> 2) >> (2u * (k & 3u))) & 3u);
    if constexpr ((FEAT & (FEAT_TEX | FEAT_EMTEX | FEAT_ENV)) != 0u) s_znodes[lane] = sc.z_nodes[lane];   // rgb2spec_lookup's z search (pt_device.hpp)
    __syncthreads();
    SamplerCtx sctx{prm.sampler, prm.seed, prm.log2_spp, prm.n_base4_digits, cam.width, dim_hash_tab, nullptr, 0u, 0u, nullptr, s_perm};
    StatCounters st{};
    unsigned long long tp[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long dvc[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // mi355pt_stats.divergence[4..11]
    unsigned long long t_loop0 = 0;
    uint32_t n_early = 0u;                                          // wave-uniform: rays not traced (EARLY PATH END; the kernels with one tail queue)
    if (STATS) t_loop0 = __builtin_amdgcn_s_memtime();

    for (;;) {
        if (lane == 0) s_work = atomicAdd(work_counter, 1u);
        __syncthreads();
        const uint32_t work = s_work;
        __syncthreads();
        if (work >= prm.n_work) break;
        // this lane's own pixel of the tile (film write-back) and the work item's wave-uniform sample range
        const LaneJob job = PT_LANE_JOB(work, lane, cam, prm);
        const LaneJob job0 = PT_LANE_JOB(work, 0u, cam, prm);
        const uint32_t blk_log2 = prm.block_log2, blk_mask = (1u << blk_log2) - 1u;
        const uint32_t s_prefix = prm.sample_prefix_digits;
        // (the tables hold the permuted prefix in 27 bits per entry: a launch shape whose prefix is wider hashes every digit instead)
        const uint32_t hi_first_w = sobol_hi_first(prm.log2_spp, blk_log2) - s_prefix, hi_shift_w = 2u * hi_first_w - (prm.log2_spp & 1u);
        if (prm.sampler == 1u && hi_first_w < prm.n_base4_digits && hi_first_w >= 3u &&
            2u * prm.n_base4_digits - (prm.log2_spp & 1u) <= hi_shift_w + 27u) {
            // block-uniform Sobol digit prefixes: lane d computes dimension d for this block (lane 0's pixel is the block origin).
            // Single-pixel items over an aligned 4^m block of sample indices: the sample digits above m are part of the prefix.
            sctx.hi_first = sobol_hi_first(prm.log2_spp, blk_log2) - s_prefix;
            sctx.hi_shift = 2u * sctx.hi_first - (prm.log2_spp & 1u);
            const uint32_t tile_m = (encode_morton2_u32(job0.px, job0.py) << prm.log2_spp) | (s_prefix ? job0.s_cur : 0u);
            for (uint32_t dmn = lane; dmn < (uint32_t)SOBOL_HI_DIMS; dmn += 64) {
                uint32_t e = (uint32_t)(sobol_tile_hi_digits(tile_m, dmn, prm.log2_spp, prm.n_base4_digits, sctx.hi_first) >> sctx.hi_shift);   // <= 26 bits: the Morton index is a u32 and hi_shift >= 6
                const uint64_t prefix = (uint64_t)tile_m >> sctx.hi_shift;                 // the digits above digit hi_first-1
                e |= sobol_perm_index(prefix, dmn) << 27;
                uint32_t e6 = 0;
                for (uint32_t v7 = 0; v7 < 4u; ++v7) e6 |= sobol_perm_index((prefix << 2) | v7, dmn) << (5u * v7);
                s_hi[dmn] = e; s_p6[dmn] = e6;
            }
            sctx.hi_lds = s_hi; sctx.p6_lds = s_p6;
        }
        // the item's camera-ray candidates: every lane walks the tree against the block's pyramid with the same arguments (the links pending
        // in s_ring: no traversal is in flight between items), so the wave runs the walk uniformly and all lanes store the same list
        uint32_t cam_n = CAM_LIST_NONE;                            // wave-uniform: candidates in s_cand, or none (no list: overflow, switched off)
        if constexpr (CAMLIST) {
            if (sc.cam_lists != 0u) {
                const uint32_t x0 = PT_CAM_UNIFORM(job0.px), y0 = PT_CAM_UNIFORM(job0.py);
                const CamWalk cw = cam_walk(sc.nodes4, sc.root4, sc.tris, sc.tri_shift, cam_pyramid(cam, x0, y0, x0 + blk_mask, y0 + blk_mask), s_cand, CAM_LIST_CAP, s_ring);
                cam_n = PT_CAM_UNIFORM(cw.overflow ? CAM_LIST_NONE : cw.count);
            }
        }
        // The work item's paths form a pool of (pixel, sample) pairs, sample-major.  A lane whose path ended takes the next pair,
        // whichever pixel of the tile it belongs to: no lane idles while another still has samples of "its" pixel to do.  The
        // tile's film lives in LDS (ds_add_f32); the hand-out order is a function of the wave's own deterministic schedule.
        if (lane < PT_FILM_PIX) { s_film[3 * lane] = 0.0f; s_film[3 * lane + 1] = 0.0f; s_film[3 * lane + 2] = 0.0f; }
        __syncthreads();
        const uint32_t n_s = job0.s_end > job0.s_cur ? job0.s_end - job0.s_cur : 0u;
        const uint32_t pool_size = n_s << (2u * blk_log2);
        uint32_t pool_next = 0u;                                   // wave-uniform
        uint32_t my_pix = lane;
        Path P{};
        park(P);
        bool active = false;
        constexpr bool MERGED = merged_traversal<FEAT, MODE>();
        ShadowReq sh{};                                            // merged form: the light connection of the vertex just shaded, traced together with the NEXT closest-hit ray
        // merged form: a path that ended with a light connection pending stays for one more iteration (`dying`) in which only the connection
        // is traced, instead of a separate any-hit traversal at the end of the iteration (rare; keeps one traversal instance in the kernel);
        bool dying = false, susp = false;                         // (`susp`, `carry`: always false / unused — left-overs, see trace_pair_coop)
        CarryState carry{0ull};
        constexpr bool TAILQ = !STATS && tail_queue<FEAT, MODE>();       // (the instrumented kernels keep the plain shading stage)
        constexpr uint32_t DEFER = TAILQ ? 0u : defer_classes<FEAT, MODE>();
        float4* const q_base = (DEFER != 0u || TAILQ) ? defer_buf + (size_t)blockIdx.x * (queue_bytes_per_wave(STATS, FEAT, MODE) / 16u) : nullptr;     // this wave's queue(s)
        uint32_t q_head = 0u, q_tail = 0u;                         // the deferral queue (a ring); wave-uniform; the queue is empty between work items
        uint32_t q_count = 0u, q2_count = 0u;                      // the tail queue(s) (stacks, tail_queue_plan.hpp): records waiting; wave-uniform; 0 between work items
        // tail queue: a second queue for the paths whose hit is on a sort class of its own (defer_classes), so that a pass shades one class
        // (the clearcoat material in the kernels that have it: its branch is the long one.  A second queue for every class but plain Lambert
        // was measured on the kernels without clearcoat and LOSES — scene 3 2 312 -> 2 063, scene 8 2 097 -> 1 932: a class that is a tenth of
        // the hits fills its queue every ~16 iterations and leaves up to 63 paths to be bounced out in sparse passes when a work item ends)
        constexpr uint32_t TQ_CLASSES = (TAILQ && (FEAT & FEAT_CC) != 0u) ? ((1u << MT_CLEARCOAT) | (1u << (MT_CLEARCOAT | 8u))) : 0u;
        // entries per stack: with one queue at most 127 paths ever wait (a pass starts at 64, an iteration adds at most 64 and every lane is
        // free after the front), with two at most 191 in both together — the smaller stack keeps the records closer to the L2
        constexpr uint32_t QR = (TQ_CLASSES != 0u) ? QUEUE_RING : PT_TAILQ_RING1;
        // STAGING (one queue only; tail_queue_plan.hpp): when a pass follows the front in the same iteration, the records the front pushes
        // are all among the ones that pass pops, so they go through LDS instead of the global stack — through s_stack, which only the
        // traversals use and which holds nothing between two of them (cam_walk keeps its links in s_ring; the carry-over that resumed a
        // traversal from its stack is dead).  Same layout as in memory, field-major over 64 slots: float4 k of slot s at dword (k * 64 + s) * 4.
        // The two-queue kernels cannot: their class-2-first rule lets a pass leave fresh records of the other class behind.
        constexpr bool STAGE = TAILQ && TQ_CLASSES == 0u;
        static_assert(STACK_DEPTH * 64 >= (int)(TQ_STAGE_SLOTS * TQ_F4 * 4u) && TQ_STAGE_SLOTS == 64u, "a pass's worth of staged tail-queue records fits the traversal stack's LDS");
        float4* const s_stage = (float4*)s_stack;
        // LIGHT-HIT QUEUE (pt_kernel.hpp; one queue only, like the staging): the paths that arrive at an emitter wait on a stack of their own
        // behind the tail queue's, field-major over LQ_SLOTS (float4 k of slot s at lq_base + k * LQ_SLOTS + s), and are evaluated and
        // finished 64 at a time.  sc.light_queue == 0 (launch_plan.hpp use_light_queue): in place, in the front.
        constexpr bool LIGHTQ = STAGE && light_queue_of(FEAT, MODE);
        float4* const lq_base = LIGHTQ ? q_base + TQ_F4 * PT_TAILQ_RING1 : nullptr;
        uint32_t lq_count = 0u;                                    // records waiting; wave-uniform; 0 between work items
        // the record: what emitter_hit reads and what finishing the sample needs (the sampler's state, the depth and the throughput's update are not: the path ends)
        auto lq_put = [&](float4* r, const Path& Q, const Hit& h, uint32_t pix) {
            const uint32_t fl = (Q.wl.term ? 1u : 0u) | (Q.from_camera ? 2u : 0u) | (Q.prev_spec ? 4u : 0u) | ((pix & 63u) << 3);
            r[0u * LQ_SLOTS] = make_float4(__uint_as_float(Q.smp.morton), __uint_as_float(fl), Q.wl.lam0, __uint_as_float(h.tri));
            r[1u * LQ_SLOTS] = make_float4(Q.T[0], Q.T[1], Q.T[2], Q.T[3]);
            r[2u * LQ_SLOTS] = make_float4(Q.L[0], Q.L[1], Q.L[2], Q.L[3]);
            r[3u * LQ_SLOTS] = make_float4(Q.pf[0], Q.pf[1], Q.pf[2], Q.pf[3]);
            r[4u * LQ_SLOTS] = make_float4(Q.rd.x, Q.rd.y, Q.rd.z, Q.p_pdf);
            r[5u * LQ_SLOTS] = make_float4(Q.prev_pos.x, Q.prev_pos.y, Q.prev_pos.z, h.b0);
            r[6u * LQ_SLOTS] = make_float4(h.b1, h.b2, 0.0f, 0.0f);
        };
        while (true) {
            unsigned long long ts0 = 0, ts1 = 0, ts2 = 0, ts3 = 0, ts4 = 0, tsa = 0, tsb = 0;
            uint32_t bsdf_classes = 0u;
            if (STATS) ts0 = __builtin_amdgcn_s_memtime();
            bool popped = false;                            // deferral queue: this lane took a queued path (in the second shading pass)
            uint32_t pop_e = 0u;
            const unsigned long long m_needy = __ballot(!active);
            if (m_needy != 0ull && pool_next < pool_size) {
                const uint32_t idx = pool_next + rank_below(m_needy);
                if (!active && idx < pool_size) {
                    const uint32_t pix = idx & ((1u << (2u * blk_log2)) - 1u);
                    const uint32_t px = job0.px + (pix & blk_mask), py = job0.py + (pix >> blk_log2);
                    const uint32_t smp_i = job0.s_cur + (idx >> (2u * blk_log2));
                    const bool valid = px < cam.width && py < cam.height;
                    if (valid) { active = true; my_pix = pix; regen_path<STATS>(P, sctx, cam, px, py, smp_i, st); }
                }
                pool_next = min(pool_next + (uint32_t)__popcll(m_needy), pool_size);
            }
            if (!__any(active)) {
                if (pool_next >= pool_size && q_tail == q_head && (q_count | q2_count | lq_count) == 0u) break;   // (light-hit records left: one more iteration, rayless, whose front is followed by the last pass)
                // (queued paths are taken AFTER the shading stage: with nothing left to start, an iteration without rays still has to get there)
                if (!((DEFER != 0u || TAILQ) && pool_next >= pool_size)) continue;
            }
            if (STATS) { ts1 = __builtin_amdgcn_s_memtime(); if (lane == 0) st.w[4]++; if (active) st.w[5]++; }
            Hit hit{};
            bool got = false;
            const bool canonical = STATS && prm.stats_mode == 1u;                    // plain per-lane traversals in the reference's order (step counts)
            if (canonical) { if (active) got = trace_closest<STATS>(sc, P.ro, P.rd, 3.402823466e+38f, stack, hit, st); }
            else if constexpr (MERGED) {
                // ONE traversal for this iteration's closest-hit rays and the light connections the previous shading left pending
                bool occluded = false;
                if (STATS && sh.on) st.w[6]++;
                // a fresh camera ray of an item with a candidate list takes its hit from the list (below) and stays out of the traversal;
                // an iteration with no other ray — most of the iterations that start new paths — has no traversal at all
                bool cam_ray = false;
                if constexpr (CAMLIST) cam_ray = cam_n != CAM_LIST_NONE && active && !dying && P.from_camera && P.depth == 0u;
                if (!CAMLIST || __ballot((active && !dying && !popped && !cam_ray) || sh.on) != 0ull) {
                    PT_PRIO_TRAV_ENTER;
                    trace_pair_coop<STATS>(sc, P.ro, P.rd, active && !dying && !popped && !cam_ray, sh.o, sh.d, sh.t, sh.on, stack, lane, pair_lds, hit, got, occluded, st, &carry, susp, &susp);
                    PT_PRIO_TRAV_EXIT;
                }
                if constexpr (CAMLIST) {
                    if (__ballot(cam_ray) != 0ull) {
                        // what the traversal computes for such a ray: the ring flush's test (same function, same inputs, the limit the first
                        // flush sees) on every triangle the ray can hit, the minimum of the merge's key (t bits << 32 | triangle), winner_hit.
                        // The candidate is wave-uniform: its vertices come through uniform-address loads
                        const RaySetup rs = setup_ray(P.rd);
                        const f3 o2 = tri_origin(sc, P.ro);
                        unsigned long long key = (0x7f7fffffull << 32) | 0xffffffffull;                 // (FLT_MAX, no triangle)
                        for (uint32_t i = 0u; i < cam_n; ++i) {
                            const uint32_t tri = PT_CAM_UNIFORM(s_cand[i]);
                            const TriVerts tv = load_tri(sc.tris, tri);
                            float t, b0, b1, b2;
                            if (intersect_triangle<false>(o2, P.rd, rs.kx, rs.ky, rs.kz, rs.sx, rs.sy, rs.sz, 3.402823466e+38f, tv, t, b0, b1, b2)) {
                                const unsigned long long k = ((unsigned long long)__float_as_uint(t) << 32) | (unsigned long long)tri;
                                key = k < key ? k : key;
                            }
                        }
                        if (cam_ray) {
                            got = (uint32_t)key != 0xffffffffu;
                            if (got) winner_hit(sc, P.ro, P.rd, rs, (uint32_t)key, hit);
                        }
                    }
                }
                if (sh.on && !occluded) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) P.L[i] = P.L[i] + sh.c[i];
                }
                sh = ShadowReq{};      // consumed: every field dead from here on, for every lane — none of them is carried through the shading stage (+2 % on scenes 0 / 8)
            }
            else { PT_PRIO_TRAV_ENTER; got = trace_closest_coop<STATS>(sc, P.ro, P.rd, active, stack, lane, closest_lds, hit, st); PT_PRIO_TRAV_EXIT; }
            if (STATS) {
                // material divergence of the shading stage (mi355pt_stats.divergence): classes among the lanes that shade a surface
                const uint32_t mclass = (active && got) ? sc.materials[__float_as_uint(((const float4*)(sc.shade + hit.tri))[4].z)].type : 8u;
                uint32_t classes = 0u, largest = 0u, lanes = 0u;
                for (uint32_t c = 0u; c < 8u; ++c) {
                    const uint32_t n = (uint32_t)__popcll(__ballot(mclass == c));
                    classes += n ? 1u : 0u; largest = max(largest, n); lanes += n;
                }
                if (lane == 0 && lanes) { st.dv[0]++; st.dv[1] += classes; st.dv[2] += lanes; st.dv[3] += largest; }
                bsdf_classes = classes - (__ballot(mclass == MT_EMISSIVE) != 0ull ? 1u : 0u);
                ts2 = __builtin_amdgcn_s_memtime();
            }
            // the tail queue's record: what the back of the vertex still needs once the front has run — the spawning sample's f, pdf and the
            // vertex left are consumed by the front, from_camera / prev_spec are rewritten by the tail, the hit's t is never read: 20 dwords in
            // 5 float4 = 80 B.  The record's size is the queue's price: 128 -> 96 B was worth +6.5 % on C2 (the queues stream through L2 / HBM)
            // Layout: FIELD-major inside a stack (float4 k of entry e at stack base + k * capacity + e): the entries of one push / pop are
            // consecutive, so each of the five store / load instructions of a wave covers 64 x 16 B = eight whole 128-byte lines instead of a
            // sixth of 64 different ones (+1 ... 2 % over the record-major layout; 128 entries where one queue suffices +0.2 ... 0.8 %)
            // (tq_put / tq_get: the record at r, field k at r[k * stride] — in a global stack, or staged in LDS)
            auto tq_put = [&](float4* r, uint32_t stride, const Path& Q, const Hit& h, uint32_t pix) {
                const uint32_t fl = (Q.wl.term ? 1u : 0u) | ((Q.depth & 1023u) << 1) | ((pix & 63u) << 11) | (Q.smp.dimension << 17);   // (max_depth <= 1000, api.cpp check_args: dimension <= 3 + 8 * 1000 < 2^15)
                r[0u * stride] = make_float4(__uint_as_float(Q.smp.morton), __uint_as_float(fl), Q.wl.lam0, __uint_as_float(h.tri));
                r[1u * stride] = make_float4(Q.T[0], Q.T[1], Q.T[2], Q.T[3]);
                r[2u * stride] = make_float4(Q.L[0], Q.L[1], Q.L[2], Q.L[3]);
                r[3u * stride] = make_float4(Q.rd.x, Q.rd.y, Q.rd.z, h.b0);
                r[4u * stride] = make_float4(h.b1, h.b2, __uint_as_float(Q.smp.rkey_lo), __uint_as_float(Q.smp.rkey_hi));
            };
            auto tq_store = [&](uint32_t e, const Path& Q, const Hit& h, uint32_t pix) {
                tq_put(q_base + (size_t)(e >> 8) * (TQ_F4 * QUEUE_RING) + (e & (QR - 1u)), QR, Q, h, pix);
            };
            struct TqRec { float4 a, b, c, d, e4; };
            auto tq_get = [&](const float4* r, uint32_t stride) { return TqRec{r[0u * stride], r[1u * stride], r[2u * stride], r[3u * stride], r[4u * stride]}; };
            auto tq_unpack = [&](const TqRec& rec, Path& Q, Hit& h, uint32_t& pix) {
                const float4 a = rec.a, b = rec.b, c = rec.c, d = rec.d, e4 = rec.e4;
                const uint32_t fl = __float_as_uint(a.y);
                Q.smp.morton = __float_as_uint(a.x); Q.smp.dimension = fl >> 17; Q.smp.rkey_lo = __float_as_uint(e4.z); Q.smp.rkey_hi = __float_as_uint(e4.w);
                Q.wl.lam0 = a.z; Q.wl.term = (fl & 1u) != 0u; Q.depth = (fl >> 1) & 1023u; pix = (fl >> 11) & 63u;
                Q.from_camera = false; Q.prev_spec = false;
                Q.T[0] = b.x; Q.T[1] = b.y; Q.T[2] = b.z; Q.T[3] = b.w; Q.L[0] = c.x; Q.L[1] = c.y; Q.L[2] = c.z; Q.L[3] = c.w;
                Q.rd = mk3(d.x, d.y, d.z); Q.ro = mk3(0.0f, 0.0f, 0.0f);
                h.b0 = d.w; h.b1 = e4.x; h.b2 = e4.y; h.tri = __float_as_uint(a.w); h.mclass = 0u; h.t = 0.0f;
#pragma unroll
                for (int i = 0; i < 4; ++i) Q.pf[i] = 0.0f;
                Q.p_pdf = 0.0f; Q.prev_pos = mk3(0.0f, 0.0f, 0.0f);
            };
            auto tq_load = [&](uint32_t e, Path& Q, Hit& h, uint32_t& pix) {
                tq_unpack(tq_get(q_base + (size_t)(e >> 8) * (TQ_F4 * QUEUE_RING) + (e & (QR - 1u)), QR), Q, h, pix);
            };
            // the deferral queue's record (the instrumented kernels): the whole path, the hit and the pixel, record-major, 8 float4 = 128 B
            auto dq_store = [&](uint32_t e, const Path& Q, const Hit& h, uint32_t pix) {
                float4* r = q_base + (size_t)e * DEFER_F4;
                // (flags in bits 0-2, the depth in bits 3-12: max_depth <= 1000, api.cpp check_args; the pixel from bit 16)
                const uint32_t fl = (Q.wl.term ? 1u : 0u) | (Q.from_camera ? 2u : 0u) | (Q.prev_spec ? 4u : 0u) | ((Q.depth & 1023u) << 3) | (pix << 16);
                r[0] = make_float4(__uint_as_float(Q.smp.morton), __uint_as_float(Q.smp.dimension), __uint_as_float(Q.smp.rkey_lo), __uint_as_float(Q.smp.rkey_hi));
                r[1] = make_float4(Q.wl.lam0, __uint_as_float(fl), Q.T[0], Q.T[1]);
                r[2] = make_float4(Q.T[2], Q.T[3], Q.L[0], Q.L[1]);
                r[3] = make_float4(Q.L[2], Q.L[3], Q.rd.x, Q.rd.y);
                r[4] = make_float4(Q.rd.z, Q.pf[0], Q.pf[1], Q.pf[2]);
                r[5] = make_float4(Q.pf[3], Q.p_pdf, Q.prev_pos.x, Q.prev_pos.y);
                r[6] = make_float4(Q.prev_pos.z, h.t, h.b0, h.b1);
                r[7] = make_float4(h.b2, __uint_as_float(h.tri), __uint_as_float(h.mclass), 0.0f);
            };
            auto dq_load = [&](uint32_t e, Path& Q, Hit& h, uint32_t& pix) {
                const float4* r = q_base + (size_t)e * DEFER_F4;
                const float4 a = r[0], b = r[1], c = r[2], d = r[3], e4 = r[4], f = r[5], g = r[6], h4 = r[7];
                const uint32_t fl = __float_as_uint(b.y);
                Q.smp.morton = __float_as_uint(a.x); Q.smp.dimension = __float_as_uint(a.y); Q.smp.rkey_lo = __float_as_uint(a.z); Q.smp.rkey_hi = __float_as_uint(a.w);
                Q.wl.lam0 = b.x; Q.wl.term = (fl & 1u) != 0u; Q.from_camera = (fl & 2u) != 0u; Q.prev_spec = (fl & 4u) != 0u; Q.depth = (fl >> 3) & 1023u; pix = fl >> 16;
                Q.T[0] = b.z; Q.T[1] = b.w; Q.T[2] = c.x; Q.T[3] = c.y; Q.L[0] = c.z; Q.L[1] = c.w; Q.L[2] = d.x; Q.L[3] = d.y;
                Q.rd = mk3(d.z, d.w, e4.x); Q.ro = mk3(0.0f, 0.0f, 0.0f);
                Q.pf[0] = e4.y; Q.pf[1] = e4.z; Q.pf[2] = e4.w; Q.pf[3] = f.x; Q.p_pdf = f.y; Q.prev_pos = mk3(f.z, f.w, g.x);
                h.t = g.y; h.b0 = g.z; h.b1 = g.w; h.b2 = h4.x; h.tri = __float_as_uint(h4.y); h.mclass = __float_as_uint(h4.z);
            };
            auto finish_path = [&]() {            // Sensor::add_sample of a finished path into the work item's LDS film tile (+ the per-sample log)
                if (pout.L != nullptr) {
                    const uint32_t px = job0.px + (my_pix & blk_mask), py = job0.py + (my_pix >> blk_log2);
                    const uint32_t tile_k = (work / prm.chunks) >> (6u - 2u * blk_log2);
                    const uint32_t smp_i = P.smp.morton & ((1u << prm.log2_spp) - 1u);
                    sample_log(P, pout, ((size_t)tile_k * 64u + ((py & 7u) * 8u + (px & 7u))) * pout.n_s + (smp_i - pout.s_base));
                }
                float r, g, b;
                film_rgb(P, sc, prm, r, g, b);
                atomicAdd(&s_film[3 * my_pix], r); atomicAdd(&s_film[3 * my_pix + 1], g); atomicAdd(&s_film[3 * my_pix + 2], b);
            };
            if constexpr (TAILQ) {
                // front of the vertex for every lane that traced: does the path go on?
                bool end_path = dying;                         // (a dying path's last connection has just been resolved)
                const bool front = active && !dying && !susp;
                unpark(P);
                // the paths that arrive at an emitter end there: they wait in the light-hit queue, and their lanes are free
                // (an emitter hit that contributes nothing — NEE after a non-specular bounce — is not queued: the front ends it unevaluated)
                // (they skip the front — no throughput update, no roulette draw for a path that ends regardless — and are stored below, with the
                // tail queue's pushes: one release for both.  sc.light_queue == 0: not stored; they keep their lanes, which evaluate them
                // below, in place, from their registers — the same statements the pass runs.  lq_void: an emitter hit that adds nothing ends here)
                bool lq_push = false, lq_void = false;
                if constexpr (LIGHTQ) {
                    const bool on_emitter = front && got && (hit.mclass & 7u) == MT_EMISSIVE;
                    lq_void = on_emitter && emitter_hit_is_void<STATS>(prm, P.from_camera, P.prev_spec);
                    lq_push = on_emitter && !lq_void;
                }
                const unsigned long long m_lq = (LIGHTQ && sc.light_queue != 0u) ? __ballot(lq_push) : 0ull;
                {
                    ShadeCtx C0;
                    C0.cont = false;
                    if constexpr (LIGHTQ) {
                        // (PHASE 4: the roulette of this vertex was decided, draw included, by the pass that spawned the ray — EARLY PATH END below)
                        if (front && !lq_push && !lq_void) end_path = shade_vertex_head<STATS, FEAT, 4>(P, sc, prm, sctx, got, hit, sh, st, tsa, C0);
                        if (lq_void) end_path = true;
                    } else {
                        if (front) end_path = shade_vertex_head<STATS, FEAT, 1>(P, sc, prm, sctx, got, hit, sh, st, tsa, C0);
                    }
                }
                dying = false;
                // the paths that go on wait in the queue of their sort class; their lanes are free
                const bool go_on = front && !lq_push && !end_path;
                const bool cls2 = TQ_CLASSES != 0u && ((TQ_CLASSES >> (hit.mclass & 31u)) & 1u) != 0u;
                const unsigned long long m_on1 = __ballot(go_on && !cls2), m_on2 = TQ_CLASSES != 0u ? __ballot(go_on && cls2) : 0ull;
                // one queue: a pass is due after this push?  Then it takes every record of the push, and they wait in LDS (wave-uniform;
                // sc.queue_stage == 0, launch_plan.hpp use_queue_staging: everything through the global stack)
                // (`if constexpr`: not a statement of this may reach the two-queue kernels, whose schedule is measured as it is)
                uint32_t n_on1 = 0u;
                bool stage = false;
                if constexpr (STAGE) {
                    n_on1 = (uint32_t)__popcll(m_on1);
                    stage = sc.queue_stage != 0u && tq_stage_pushes(q_count, n_on1, pool_next >= pool_size, (uint32_t)PT_TAILQ_MIN);
                }
                if ((m_on1 | m_on2 | m_lq) != 0ull) {
                    if constexpr (LIGHTQ) {
                        if (lq_push && m_lq != 0ull) {
                            lq_put(lq_base + (lq_push_slot(lq_count, rank_below(m_lq)) & (LQ_SLOTS - 1u)), P, hit, my_pix);
                            active = false;
                        }
                        lq_count += (uint32_t)__popcll(m_lq);
                    }
                    if (go_on) {
                        if (STAGE && stage) tq_put(s_stage + tq_stage_push_index(rank_below(m_on1)), TQ_STAGE_SLOTS, P, hit, my_pix);
                        else {
                            // (on top of the stack: consecutive ranks, consecutive entries)
                            const uint32_t e = cls2 ? QUEUE_RING + tq_push_slot(q2_count, rank_below(m_on2)) : tq_push_slot(q_count, rank_below(m_on1));
                            tq_store(e, P, hit, my_pix);
                        }
                        active = false;
                    }
                    q_count += (uint32_t)__popcll(m_on1); q2_count += (uint32_t)__popcll(m_on2);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                }
                if (active && end_path) { finish_path(); active = false; }
                park(P, false);                                 // (nothing of these lanes' records is needed any more: the queue has them)
                // The emitter hits.  With the queue: every lane is free and no path state is live — do 64 records wait, or is the work item
                // done and some are left?  Then a pass: the newest min(64, count), one per lane.  Without it: the lanes that arrived at an
                // emitter, as they stand.  Either way emitter_hit and what finish_path does, in ONE place
                if constexpr (LIGHTQ) {
                    bool ev = lq_push;
                    if (sc.light_queue != 0u) {
                        ev = false;
                        if (lq_pass_due(lq_count, pool_next >= pool_size && q_count == 0u)) {
                            const uint32_t n = lq_pass_take(lq_count);
                            ev = lane < n;
                            if (ev) {
                                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                                const float4* r = lq_base + (lq_pop_slot(lq_count, n, lane) & (LQ_SLOTS - 1u));
                                const float4 a = r[0u * LQ_SLOTS], b = r[1u * LQ_SLOTS], c = r[2u * LQ_SLOTS], d = r[3u * LQ_SLOTS], e4 = r[4u * LQ_SLOTS], f = r[5u * LQ_SLOTS], g = r[6u * LQ_SLOTS];
                                const uint32_t fl = __float_as_uint(a.y);
                                P.smp.morton = __float_as_uint(a.x); P.wl.lam0 = a.z; P.wl.term = (fl & 1u) != 0u;
                                P.from_camera = (fl & 2u) != 0u; P.prev_spec = (fl & 4u) != 0u; my_pix = (fl >> 3) & 63u;
                                P.T[0] = b.x; P.T[1] = b.y; P.T[2] = b.z; P.T[3] = b.w; P.L[0] = c.x; P.L[1] = c.y; P.L[2] = c.z; P.L[3] = c.w;
                                P.pf[0] = d.x; P.pf[1] = d.y; P.pf[2] = d.z; P.pf[3] = d.w;
                                P.rd = mk3(e4.x, e4.y, e4.z); P.p_pdf = e4.w; P.prev_pos = mk3(f.x, f.y, f.z);
                                hit.b0 = f.w; hit.b1 = g.x; hit.b2 = g.y; hit.tri = __float_as_uint(a.w);
                            }
                            lq_count -= n;
                        }
                    }
                    if (ev) {
                        emitter_hit<STATS, FEAT>(sc, prm, hit, P.rd, P.T, P.pf, P.p_pdf, P.prev_pos, P.wl, P.from_camera, P.prev_spec, P.L, st);
                        finish_path();
                        active = false;
                    }
                }
                if (STATS) ts3 = ts4 = __builtin_amdgcn_s_memtime();
                // the back of the vertex and its tail for a full wave of queued paths — of ONE class while new paths still arrive (the class
                // with its own queue first); when the work item has nothing new left, whatever waits in either queue shares the passes
                const bool draining = pool_next >= pool_size;
                // A pass takes the NEWEST records (tail_queue_plan.hpp): mostly the ones the front above has just stored, read back while their
                // lines are still in the L2, instead of the oldest, written an iteration or two ago and evicted since
                if (tq_pass_due(q_count, q2_count, draining, TQ_CLASSES != 0u, (uint32_t)PT_TAILQ_MIN)) {
                    const unsigned long long m_free = __ballot(!active);
                    const uint32_t n_free = (uint32_t)__popcll(m_free), r = rank_below(m_free);
                    // lanes 0 .. n2-1 of the free lanes take from queue 2, the next n1 from queue 1
                    const TqTake tk = tq_pass_take(q_count, q2_count, n_free, draining, TQ_CLASSES != 0u, (uint32_t)PT_TAILQ_MIN);
                    const uint32_t n2 = tk.n2, n1 = tk.n1;
                    const bool take2 = !active && r < n2, take1 = !active && !take2 && r - n2 < n1;
                    const bool take = take1 || take2;
                    const uint32_t e = take2 ? QUEUE_RING + tq_pop_slot(q2_count, n2, r) : tq_pop_slot(q_count, n1, r - n2);
                    // (one queue: the same slot, and where it is — the records staged above lie on top of the q_count - n_on1 older ones)
                    TqStagePop sp{0u, false, 0u};
                    if constexpr (STAGE) sp = tq_stage_pop(stage ? q_count - n_on1 : q_count, stage ? n_on1 : 0u, n1, r - n2);
                    q2_count -= n2; q_count -= n1;
                    bool ep = false;
                    bool ended_early = false;                       // (one queue: this lane's path ended without its last ray, EARLY PATH END below)
                    if constexpr ((FEAT & FEAT_CC) != 0u) {
                        ShadeCtx C;
                        shade_ctx_idle_cc(C);
                        if (take) {
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                            tq_load(e, P, hit, my_pix);
                            active = true;
                            shade_vertex_head<STATS, FEAT, 2>(P, sc, prm, sctx, true, hit, sh, st, tsa, C);
                        }
                        // the coat's 64-sample directional albedo, estimated by the whole wave for the lanes that need it
                        const bool want_mc = take && C.cont && C.need_cc;
                        const float fc_mc = coat_directional_albedo_coop(want_mc, C.cc_alpha_c, C.cc_r0c, C.wo_nm, C.mc_key, lane);
                        if (want_mc) C.cc_fc = fc_mc;
                        if (take && C.cont) ep = shade_vertex_tail<STATS, FEAT>(P, sc, prm, sctx, sh, st, tsb, C);
                    } else if (take) {
                        // (ONE divergent region for the back of the head and the tail: ShadeCtx must not cross a re-convergence point in the
                        // kernels that run 4 waves per SIMD — the split form of this block cost them 12 %)
                        // (the older records from the global stack, the staged ones from LDS: written global side first, but the compiler
                        // orders the two sides of the branch itself and puts the five LDS reads first — one LDS round trip per mixed pass)
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                        static_assert(STAGE, "the kernels without the clearcoat code have one queue");
                        TqRec rec;
                        if (!sp.staged) rec = tq_get(q_base + sp.slot, QR);
                        else rec = tq_get(s_stage + sp.index, TQ_STAGE_SLOTS);
                        tq_unpack(rec, P, hit, my_pix);
                        active = true;
                        ShadeCtx C;
                        C.cont = false; C.need_cc = false; C.cc_fc = 0.0f;
                        shade_vertex_head<STATS, FEAT, 2>(P, sc, prm, sctx, true, hit, sh, st, tsa, C);
                        if (C.cont) ep = shade_vertex_tail<STATS, FEAT>(P, sc, prm, sctx, sh, st, tsb, C);
                        // EARLY PATH END (path_end_plan.hpp).  The roulette and the depth test of the NEXT vertex read nothing the ray finds: the
                        // decision is taken here, and the draw made here, at the dimension the front would have drawn at.  A doomed path's ray can
                        // only add an emitter's radiance to L (or the NaN of a non-finite throughput): when it can do neither — no environment
                        // light, the non-emitter term an exact zero, the ray past every area light's padded box; under NEE after a non-specular
                        // sample an emitter adds nothing either — the path ends now, as one whose BSDF sample failed ends (`dying` below, if a
                        // connection is pending).  Every other doomed path is traced and carries the decision to its front (PHASE 4).
                        // sc.early_path_end == 0 (launch_plan.hpp use_early_path_end): same decision, same draw, every ray traced.
                        if (C.cont && !ep) {
                            const float p_next = path_end_pmax(P.T, P.pf, P.p_pdf);
                            float ur = 0.0f;
                            if (path_end_draws(p_next, prm.rr_gate)) ur = get_1d(P.smp, sctx);
                            if (path_end_doomed(p_next, ur, prm.rr_gate, P.depth, prm.max_depth)) {
                                P.depth |= PATH_DOOMED_BIT;
                                bool skip = sc.early_path_end != 0u && sc.n_envs == 0u;
                                if (skip && !emitter_hit_is_void<STATS>(prm, false, P.prev_spec)) {
                                    const float w = (prm.strategy == 2u && !P.prev_spec) ? balance_heuristic(P.p_pdf, 0.0f) : 1.0f;   // the front's
                                    skip = path_end_term_is_zero(P.T, w);
                                    const float o[3] = {P.ro.x, P.ro.y, P.ro.z}, d[3] = {P.rd.x, P.rd.y, P.rd.z};
                                    for (uint32_t li = 0u; li < sc.n_lights; ++li) {          // wave-uniform records
                                        const float4* bx = (const float4*)light_box_of(sc.lights, sc.n_lights, li);
                                        const float4 b0 = bx[0], b1 = bx[1];
                                        const float lo[3] = {b0.x, b0.y, b0.z}, hi[3] = {b1.x, b1.y, b1.z};
                                        if (light_box_may_reach(o, d, lo, hi, b0.w)) skip = false;
                                    }
                                }
                                if (skip) { ep = true; ended_early = true; }
                            }
                        }
                    }
                    if constexpr (STAGE) n_early += (uint32_t)__popcll(__ballot(ended_early));
                    park(P, take);
                    if (sh.on && sh.c[0] == 0.0f && sh.c[1] == 0.0f && sh.c[2] == 0.0f && sh.c[3] == 0.0f) sh.on = false;
                    if (!active) sh.on = false;
                    // (a path that ended early keeps its lane until the next front, connection or not, like the doomed path it was: a lane freed
                    // here starts a camera path in the iteration that follows a pass, where no other lane is free — the hand-out, the Sobol
                    // prefixes and the candidate test for a handful of lanes, every cycle.  Measured: with the lanes freed C2 LOSES 3.3 %)
                    if (take) { dying = (sh.on && ep) || ended_early; if (dying) ep = false; }
                    if (take && ep) { finish_path(); active = false; }
                }
            } else
            // The shading stage.  It runs a second time in the iterations that shade the deferral queue: the lanes the first pass freed
            // (ended paths, deferred hits) take queued paths and shade them at once, so a queued path rejoins the NEXT traversal with its
            // next ray like everybody else.
            for (int pass = 0;; ++pass) {
            const bool mine = pass == 0 || popped;     // the lanes this pass works on
            bool end_path = pass == 0 && MERGED && dying;           // a dying path's last connection has just been resolved
            if (pass == 0) {
                if constexpr (!MERGED) sh = ShadowReq{};
                unpark(P);
            }
            if constexpr (DEFER != 0u) {
                // queued paths join here: path state, hit and pixel of the lanes that popped
                if (popped) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    dq_load(pop_e, P, hit, my_pix);
                    got = true;
                }
                // and the lanes whose hit is on a deferred material leave
                const bool defer_now = pass == 0 && !(STATS && prm.stats_mode == 1u) && active && !dying && !susp && !popped && got && ((DEFER >> (hit.mclass & 31u)) & 1u) != 0u;
                const unsigned long long m_def = __ballot(defer_now);
                if (m_def != 0ull) {
                    if (defer_now) {
                        dq_store((q_tail + rank_below(m_def)) & (DEFER_RING - 1u), P, hit, my_pix);
                        active = false;                                      // free: a new path (or a queued one) next
                    }
                    q_tail += (uint32_t)__popcll(m_def);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                }
            }
            const bool shade_now = mine && active && !(MERGED && (dying || susp));
            if constexpr ((FEAT & FEAT_CC) != 0u) {
                ShadeCtx C;
                shade_ctx_idle_cc(C);
                if (shade_now) end_path = shade_vertex_head<STATS, FEAT>(P, sc, prm, sctx, got, hit, sh, st, tsa, C);
                // the coat's 64-sample directional albedo, estimated by the whole wave for the lanes that need it
                const bool want_mc = shade_now && C.cont && C.need_cc;
                const float fc_mc = coat_directional_albedo_coop(want_mc, C.cc_alpha_c, C.cc_r0c, C.wo_nm, C.mc_key, lane);
                if (want_mc) C.cc_fc = fc_mc;
                if (shade_now && C.cont) end_path = shade_vertex_tail<STATS, FEAT>(P, sc, prm, sctx, sh, st, tsb, C);
            } else {
                if (shade_now) end_path = shade_vertex<STATS, FEAT>(P, sc, prm, sctx, got, hit, sh, st, tsa, tsb);
            }
            park(P, mine);
            if (STATS) {
                ts3 = __builtin_amdgcn_s_memtime();
                // the stamps inside shade_vertex are taken by the lanes that reach them: make them wave-level (first lane that has one)
                unsigned long long ma = __ballot(tsa != 0ull), mb = __ballot(tsb != 0ull);
                if (ma) { int l = (int)__ffsll((long long)ma) - 1; tsa = ((unsigned long long)__shfl((uint32_t)(tsa >> 32), l) << 32) | __shfl((uint32_t)tsa, l); }
                if (mb) { int l = (int)__ffsll((long long)mb) - 1; tsb = ((unsigned long long)__shfl((uint32_t)(tsb >> 32), l) << 32) | __shfl((uint32_t)tsb, l); }
            }
            // a light connection whose contribution is exactly zero (light behind the surface, f == 0) cannot change L whatever the
            // visibility test says: the production path does not trace it (the canonical-count mode does, like the reference)
            if (!canonical && sh.on && sh.c[0] == 0.0f && sh.c[1] == 0.0f && sh.c[2] == 0.0f && sh.c[3] == 0.0f) sh.on = false;
            if (!active) sh.on = false;
            if (MERGED && !canonical) {
                // merged form: the connection of a CONTINUING path waits for the next iteration's traversal; a path that ends here with a
                // connection pending (a failed BSDF sample after the light was sampled: rare) lives on for that traversal alone
                if (mine) {
                    dying = sh.on && end_path;
                    if (dying) end_path = false;
                }
            } else {
                // two traversals per iteration — and everything in the canonical-count mode: the connection is traced now
                const bool now = sh.on;
                if (__any(now)) {
                    if (STATS && now) st.w[6]++;
                    bool occluded = false;
                    if (canonical) { if (now) occluded = trace_any<STATS>(sc, sh.o, sh.d, sh.t, stack, st); }
                    else { PT_PRIO_TRAV_ENTER; occluded = trace_any_deferred<STATS>(sc, sh.o, sh.d, sh.t, now, stack, lane, any_lds, st); PT_PRIO_TRAV_EXIT; }
                    if (now && !occluded) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) P.L[i] = P.L[i] + sh.c[i];
                    }
                    if (now) sh.on = false;
                }
            }
            if (STATS) ts4 = __builtin_amdgcn_s_memtime();
            if (mine && active && end_path) {
                if (pout.L != nullptr) {
                    // per-sample log (see PathOut): the sample index is the low log2(spp) bits of the lane's Morton index (spp a power of two)
                    const uint32_t px = job0.px + (my_pix & blk_mask), py = job0.py + (my_pix >> blk_log2);
                    const uint32_t tile_k = (work / prm.chunks) >> (6u - 2u * blk_log2);
                    const uint32_t smp_i = P.smp.morton & ((1u << prm.log2_spp) - 1u);
                    sample_log(P, pout, ((size_t)tile_k * 64u + ((py & 7u) * 8u + (px & 7u))) * pout.n_s + (smp_i - pout.s_base));
                }
                float r, g, b;
                film_rgb(P, sc, prm, r, g, b);
                atomicAdd(&s_film[3 * my_pix], r); atomicAdd(&s_film[3 * my_pix + 1], g); atomicAdd(&s_film[3 * my_pix + 2], b);
                active = false;
            }
            // a second pass for the deferral queue?
            if constexpr (DEFER != 0u) {
                if (pass != 0 || (STATS && prm.stats_mode == 1u)) break;
                const uint32_t q_count = q_tail - q_head;
                if (!(q_count >= (uint32_t)PT_DEFER_MIN || (pool_next >= pool_size && q_count != 0u))) break;
                const unsigned long long m_free = __ballot(!active);
                if (m_free == 0ull) break;
                const uint32_t r = rank_below(m_free);
                popped = !active && r < q_count;
                if (popped) { active = true; dying = false; pop_e = (q_head + r) & (DEFER_RING - 1u); }
                q_head += min((uint32_t)__popcll(m_free), q_count);
            } else break;
            }
            if (STATS) {
                unsigned long long ts5 = __builtin_amdgcn_s_memtime();
                dvc[min(bsdf_classes, 3u)] += 1ull; dvc[4 + min(bsdf_classes, 3u)] += ts3 - ts2;
                tp[0] += ts1 - ts0; tp[1] += ts2 - ts1; tp[2] += ts3 - ts2; tp[3] += ts4 - ts3; tp[4] += ts5 - ts4;
                if (tsa) { tp[6] += tsa - ts2; if (tsb) { tp[7] += tsb - tsa; tp[8] += ts3 - tsb; } else tp[7] += ts3 - tsa; } else tp[6] += ts3 - ts2;
            }
        }
        __syncthreads();
        if (job.valid) {
            size_t o = ((size_t)job.py * cam.width + job.px) * 3;
            const float fr = s_film[3 * lane], fg = s_film[3 * lane + 1], fb = s_film[3 * lane + 2];
            if (prm.chunks == 1) { accum[o] += fr; accum[o + 1] += fg; accum[o + 2] += fb; }
            else {
                // the sample range of this tile is split over several work items: each writes its own slot, combine_kernel adds the
                // slots to the film in chunk order (no float atomics: frames stay bit-identical from run to run)
                // (slots are laid out per 8x8 tile and chunk whatever the block size, see combine_kernel)
                const uint32_t tile_k = (work / prm.chunks) >> (6u - 2u * blk_log2), chunk = work % prm.chunks;
                float* slot = partial + (((size_t)tile_k * prm.chunks + chunk) * 64u + ((job.py & 7u) * 8u + (job.px & 7u))) * 3u;
                slot[0] = fr; slot[1] = fg; slot[2] = fb;
            }
        }
        __syncthreads();
    }
    if (STATS && lane == 0) {
        tp[5] = __builtin_amdgcn_s_memtime() - t_loop0;
        for (int i = 0; i < 10; ++i) atomicAdd(&stats->phase_cycles[i], tp[i]);
        for (int i = 0; i < 8; ++i) atomicAdd(&stats->divergence[4 + i], dvc[i]);
    }
    if (STATS) flush_stats(stats, st);
    // (a production launch is given a stats block only by a caller that asked for this count: api.cpp launch_range)
    if (!STATS && n_early != 0u && stats != nullptr && lane == 0) atomicAdd(&stats->wave_steps[7], (unsigned long long)n_early);
