    // rt_paths_body.inc -- the body of paths_kernel<LDS, COUNT, TEX, BLOCK> and of paths_prog_kernel<LDS, COUNT, BLOCK> (rt_paths_kernels.h),
    // included once in each.  The includer provides LDS, COUNT, TEX and BLOCK and the kernel arguments `p` and `q`.  Text and not a function,
    // for the reason rt_render_body.inc gives: paths_kernel compiles to exactly what it did when these lines stood in it.
    static_assert(!(LDS && COUNT), "the counting variant reads the exact records in global memory");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if constexpr (LDS) (void) stage_scene<BLOCK, true>(p, smem);
    const SceneView<LDS> sc = make_view<LDS, LDS>(p, smem);
    const int lane = threadIdx.x & 63;
    const uint32_t P = (uint32_t) q.chunk;
    const uint32_t K = (uint32_t) q.max_vertices;
    const bool camera = q.rays == nullptr;
    const double nanv = __builtin_nan("");
    Counters cnt; cnt.rays = cnt.aabb = cnt.prim = cnt.refl = 0;

    // the lane's path
    bool live = false;
    uint32_t slot = 0u, entry = 0u, colour = RTD_WHITE, albedo = 0u;
    int nv = 0, bounces = 0;
    V3 o = mk(0.0, 0.0, 0.0), d = mk(1.0, 0.0, 0.0);
    Rng rng; rng.x = rng.y = rng.z = rng.w = 0u;
    // wave-uniform: slots [next, stop) of the wave's current runs are not handed out yet
    uint64_t next = 0, stop = 0;
    bool exhausted = false;

    // a path's end: the per-slot outputs, once, and the records it did not reach
    auto retire = [&](int end, uint32_t result) {
        const size_t i = (size_t) slot;
        if (q.n_vertices) q.n_vertices[i] = nv;
        if (q.end) q.end[i] = end;
        if (q.colour) path_store_rgb(q.colour + i * 3, result);
        if (q.rng) { uint32_t *r = q.rng + i * 4; r[0] = rng.x; r[1] = rng.y; r[2] = rng.z; r[3] = rng.w; }
        for (uint32_t j = (uint32_t) nv; j < K; ++j) { // (nv may exceed K: nothing to fill then)
            const size_t r = i * K + j;
            if (q.hit_index) q.hit_index[r] = -1;
            if (q.strike) { q.strike[r * 3] = nanv; q.strike[r * 3 + 1] = nanv; q.strike[r * 3 + 2] = nanv; }
            if (q.colour_after) path_store_rgb(q.colour_after + r * 3, 0u);
            if (q.ray_after) for (int a = 0; a < 6; ++a) q.ray_after[r * 6 + a] = nanv;
        }
        live = false;
    };

    // Bounded by construction: a trip either takes slots from the finite queue or advances EVERY live lane by one vertex, and a path has at
    // most depth + 1 of them.  Nothing here spins or waits on another wave: the only traffic between waves is the queue's atomicAdd and
    // the summary's integer atomics.
    for (;;) {
        // ---- (a) refill: lanes whose path ended take the next slots; as many runs are taken at once as the wave has idle lanes for ----
        const unsigned long long idle = __builtin_amdgcn_ballot_w64(!live);
        const uint32_t nIdle = (uint32_t) __popcll(idle);
        if (nIdle != 0u && (next < stop || !exhausted)) {
            if (next >= stop) {
                const uint32_t want = (nIdle + P - 1u) / P; // runs
                uint32_t unit = 0;
                if (lane == 0) unit = atomicAdd(q.queue, want);
                unit = __builtin_amdgcn_readfirstlane(unit);
                const uint64_t first = (uint64_t) unit * P;
                if (first >= q.slots) exhausted = true;
                else { next = first; stop = first + (uint64_t) want * P; stop = stop < q.slots ? stop : q.slots; }
            }
            const uint32_t avail = (uint32_t) (stop - next < 64u ? stop - next : 64u);
            const uint32_t take = nIdle < avail ? nIdle : avail;
            const uint32_t rank = lane_rank(idle);
            bool fin = false;
            if (!live && rank < take) {
                slot = (uint32_t) (next + rank); // (slots <= INT32_MAX)
                colour = RTD_WHITE; nv = 0; bounces = 0; albedo = 0u;
                bool made;
                if (camera) {
                    entry = slot / (uint32_t) q.n_samples;
                    const uint32_t s = (uint32_t) q.sample_first + (slot - entry * (uint32_t) q.n_samples);
                    const uint32_t g = q.pixel_list ? (uint32_t) q.pixel_list[entry] : entry;
                    const uint32_t r = g / (uint32_t) q.cols, c = g - r * (uint32_t) q.cols;
                    rng = stream_for(pixel_key(q.seed_key, (uint64_t) g), s);
                    made = camera_ray(*q.cam, q.max_h - (int) r - 1, (int) c - q.max_w, rng, o, d); // Scene.traceOnce's ray (Scene.fs:129-143): GetTwo
                    if (q.first_ray) {
                        double *f = q.first_ray + (size_t) slot * 6;
                        f[0] = made ? o.x : nanv; f[1] = made ? o.y : nanv; f[2] = made ? o.z : nanv;
                        f[3] = made ? d.x : nanv; f[4] = made ? d.y : nanv; f[5] = made ? d.z : nanv;
                    }
                } else {
                    const double *r = q.rays + (size_t) slot * 6;
                    o = mk(r[0], r[1], r[2]);
                    if (q.rng) { const uint32_t *g = q.rng + (size_t) slot * 4; rng.x = g[0]; rng.y = g[1]; rng.z = g[2]; rng.w = g[3]; }
                    else rng = stream_for(pixel_key(q.seed_key, q.ray_base + slot), q.ray_sample);
                    made = unitise(mk(r[3], r[4], r[5]), d); // Ray.make' (Ray.fs:26-34)
                }
                if (made) live = true;
                else { d = mk(1.0, 0.0, 0.0); retire(PATH_NO_RAY, RTD_BLACK); fin = true; } // ValueNone: Black, no vertex, nothing more drawn
            }
            next += take;
            if (q.summary) path_summarise(q, fin, entry, 0, PATH_NO_RAY, 0u, RTD_BLACK);
        }
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) {
            if (next >= stop && exhausted) break;
            continue;
        }

        // ---- (b) Scene.hitObject (Scene.fs:62-91) for every live lane ----
        int obj = -1;
        double t = nanv;
        if constexpr (LDS) {
            // node_loop_lds32 is wave-cooperative: all 64 lanes enter it, the idle ones with an exhausted walk and an empty queue.  Every
            // ray here left Ray.make' or Reflection as a unit vector, which is what the `implied` shortcut of the leaf test asks for.
            Walk w;
            walk_begin(w, sc.first);
            if (!live) w.off = sc.end;
            const WalkCtx32 f = walk_ctx32(o, d, p.off.bmax);
            double bestF = __builtin_inf();
            const bool implied = p.off.box_implied != 0;
            uint32_t pend = 0u;
            for (;;) {
#ifdef RTD_STAGE_CLOCKS
                unsigned nTrips = 0u, nLanes = 0u;
                w.off = node_loop_lds32(w.off, pend, sc.end, 0, f, nTrips, nLanes);
#else
                w.off = node_loop_lds32(w.off, pend, sc.end, 0, f); // until no lane of the wave can step: walks exhausted or queues full
#endif
                if (__builtin_amdgcn_ballot_w64(pend != 0u) == 0ull) break;
                if (pend != 0u) leaf_test_object_exact<true>(sc, o, d, bestF, w, pend_pop(pend), implied);
            }
            if (live) unbounded_tests<true, false>(sc, o, d, w, cnt);
            obj = w.best; t = w.bestLen;
        } else {
            if (live) obj = hit_object<false, COUNT>(sc, o, d, t, cnt);
        }

        // ---- (c) the vertex: record, Hittable.Reflection, record; the lanes whose path ended retire ----
        bool fin = false;
        int end = PATH_MISS;
        uint32_t result = RTD_BLACK;
        if (live) {
            if (obj < 0) { retire(PATH_MISS, RTD_BLACK); fin = true; }
            else {
                const V3 sp = walk(o, d, t); // Ray.walkAlong ray bestLength (Scene.fs:91)
                if (COUNT) cnt.refl++;
                const bool absorbed = reflection<LDS, TEX>(sc, obj, sp, o, d, colour, rng);
                if ((uint32_t) nv < K) {
                    const size_t r = (size_t) slot * K + (uint32_t) nv;
                    if (q.hit_index) q.hit_index[r] = q.obj_to_orig[obj];
                    if (q.strike) { q.strike[r * 3] = sp.x; q.strike[r * 3 + 1] = sp.y; q.strike[r * 3 + 2] = sp.z; }
                    if (q.colour_after) path_store_rgb(q.colour_after + r * 3, colour);
                    if (q.ray_after) {
                        double *a = q.ray_after + r * 6;
                        a[0] = absorbed ? nanv : o.x; a[1] = absorbed ? nanv : o.y; a[2] = absorbed ? nanv : o.z;
                        a[3] = absorbed ? nanv : d.x; a[4] = absorbed ? nanv : d.y; a[5] = absorbed ? nanv : d.z;
                    }
                }
                if (nv == 0) albedo = colour;
                nv = nv + 1;
                if (absorbed) { end = PATH_STOPPED; result = colour; retire(end, result); fin = true; }
                else {
                    bounces = bounces + 1;
                    if (bounces > q.depth) { end = PATH_BOUNCE_LIMIT; result = RTD_HOTPINK; retire(end, result); fin = true; }
                }
            }
        }
        if (q.summary) path_summarise(q, fin, entry, nv, end, albedo, result);
    }

    if (COUNT) {
        const uint64_t a = wave_sum_u64(cnt.rays), b = wave_sum_u64(cnt.aabb), c = wave_sum_u64(cnt.prim), dd = wave_sum_u64(cnt.refl);
        if (lane == 0) {
            atomicAdd(&q.counters[0], (unsigned long long) a);
            atomicAdd(&q.counters[1], (unsigned long long) b);
            atomicAdd(&q.counters[2], (unsigned long long) c);
            atomicAdd(&q.counters[3], (unsigned long long) dd);
        }
    }
