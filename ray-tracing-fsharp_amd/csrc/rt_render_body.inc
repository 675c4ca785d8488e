    // rt_render_body.inc -- the body of render_kernel<LDS, COUNT, BLOCK, MODE, TEX> and of render_job_kernel<LDS, BLOCK, PASS, TEX>
    // (rt_render_kernel.h), included once in each.  The includer provides LDS, COUNT, BLOCK, MODE and TEX, the kernel argument `p`, and the
    // job policy: `constexpr bool JOB` and `const JobCtl *job` (null without a job), and `constexpr bool VIEWS` (render_views_kernel: a batch of
    // views, rt_views_plan.h -- a unit lies inside one view and `pu` is the kernel's parameters with THAT view's camera and seed key; also
    // camera_hits_views_kernel, the one includer with MODE = CAMERA_HITS and VIEWS).  Text and not a function, so that render_kernel
    // compiles to exactly what it did when these lines stood in it: as a shared inline function the same lines gave every
    // instantiation another instruction stream and 55 of the 304 other resource figures (NOTES.md, round 28).
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr rtmode::ModeDesc D = rtmode::mode_desc(MODE);
    constexpr bool FUSED = D.pass == rtmode::Pass::FUSED, PASS_A = D.pass == rtmode::Pass::A, PASS_B = D.pass == rtmode::Pass::B;
    constexpr bool RAYS = D.pass == rtmode::Pass::RAY_LIST, CAM = D.pass == rtmode::Pass::CAMERA_HITS;
    constexpr bool MAP = D.map, LOG = D.ray_log;
    constexpr bool FP = D.pixels == rtmode::Pixels::FOOTPRINTS;  // the pixels are the caller's footprints
    constexpr bool PX = D.pixels == rtmode::Pixels::LIST && !CAM; // the pixels are a caller's list of the frame's, rendered as the frame's are
    const int lane = threadIdx.x & 63;
    // the wave's index as a SCALAR: everything derived from it (the wave's LDS scratch, its park pools) then has a scalar base, and the
    // pools' field addresses are scalar base + 32-bit lane offset instead of 64-bit vector arithmetic kept alive across the loop
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));

    // LDS part: the whole scene (LDS variants), or as much of the tree as fits (the timed variant of a larger scene), or nothing
    const uint32_t ldsNodes = (!LDS && !COUNT) ? stage_nodes32<BLOCK>(p, smem) : 0u;
    const uint32_t sceneBytes = LDS ? stage_scene<BLOCK, !COUNT>(p, smem) : (uint32_t) ((!LDS && !COUNT) ? p.lds_node_bytes : 0);
    SceneView<LDS> scv = make_view<LDS, !COUNT>(p, smem);
    scv.lds_lim = (int) ldsNodes;
    scv.lds_thr = p.lds_node_thr;
    const SceneView<LDS> &sc = scv;
    const uint32_t P = (uint32_t) p.chunk;
    RTD_AS3 uint32_t *wv = (RTD_AS3 uint32_t *) (smem + sceneBytes) + (size_t) wave * rtmode::wave_words(MODE, P);
    RTD_AS3 uint32_t *acc = wv;
    RTD_AS3 uint32_t *pix = wv + 6u * P;
    RTD_AS3 uint32_t *live = pix + 4u * P;
    RTD_AS3 uint32_t *cand = live + P; // (fused and pass A; pass B keeps its own behind the two slots)
    unsigned char *pool = p.park_pool + ((size_t) blockIdx.x * (BLOCK / 64) + (size_t) wave) * (size_t) RTD_PARK_ENTRY_BYTES *
                                        (size_t) (p.park + (p.park_l_lds ? 0 : p.park_l) + (TEX ? p.park : 0));
    // the Lambert pools in LDS (if any) follow the waves' scratch
    RTD_AS3 unsigned char *poolLds = (RTD_AS3 unsigned char *) (smem + sceneBytes) + (size_t) (BLOCK / 64) * rtmode::wave_words(MODE, P) * 4u +
                                     (size_t) wave * (size_t) RTD_PARK_L_LDS_BYTES * (size_t) p.park_l;

    const uint64_t nLocal = PX ? p.ray_n : (uint64_t) p.n_rows * (uint64_t) p.cols; // (a pixel list: cols is the frame's)
    const uint32_t k = (uint32_t) p.k;
    const uint32_t n1 = (PASS_B && p.first_b != 0) ? (uint32_t) p.first_b : 2u * k + 1u; // (pass B of an extension starts where the buffer ends)
    const int n2s = p.spp - (int) n1; // Scene.fs:191
    const uint32_t n2 = n2s > 0 ? (uint32_t) n2s : 0u;

    const unsigned long long tStart = COUNT ? __builtin_amdgcn_s_memrealtime() : 0ull;
    Counters cnt; cnt.rays = cnt.aabb = cnt.prim = cnt.refl = 0;
    StageStats ss; ss.refill = ss.trips = ss.leaf = ss.shade = ss.refillLanes = ss.shadeLanes = ss.slow = ss.slowLanes = ss.parkedLanes = 0;
    ss.tRefill = ss.tSlow = ss.tWalk = ss.tShade = 0ull;
    ss.tLoop = ss.tLeaf = ss.tUnb = ss.tCam = ss.tLamb = 0ull;
    ss.loopTrips = ss.loopLanes = 0ull;
#ifdef RTD_STAGE_CLOCKS
    ss.turns = ss.lambBatches = ss.lambLanes = ss.newRefills = ss.newItems = ss.unparkL = ss.unparkA = ss.storeBlocksL = ss.storeLanesL = ss.storeBlocksA = 0u;
    ss.lightBatches = ss.lightLanes = ss.missLanes = ss.ranges = ss.flushes = ss.leafLanes = ss.unparkBatchesL = ss.unparkBatchesA = 0u;
    for (int i = 0; i < 8; ++i) ss.slowLanesByStyle[i] = ss.slowBatchesByStyle[i] = 0u;
#endif
    uint32_t earlyCount = 0;
    uint64_t sampleCount = 0; // Scene.traceOnce calls = sum of PixelStats.Count

    if constexpr (RAYS) run_rays<LDS, COUNT, TEX, D.hits>(p, sc, pool, poolLds, cnt, ss);
    else if constexpr (CAM) run_camera_hits<LDS, COUNT, VIEWS>(p, sc, pool, poolLds, wv, cnt, ss);
    else if (PASS_B) run_stream<LDS, COUNT, TEX, FP, MAP, PX, JOB, VIEWS>(p, sc, pool, poolLds, wv, n1, n2, cnt, ss, sampleCount, job);
    else {
    std::conditional_t<VIEWS, RenderParams, const RenderParams &> pu = p;
    for (;;) {
        uint32_t unit = 0;
        if constexpr (JOB) { // (a stop: as a unit beyond the frame; the counter is left alone, so it counts the units rendered)
            if (lane == 0) unit = job_stop_requested(*job) ? 0xFFFFFFFFu : atomicAdd(p.queue, 1u);
        } else if (lane == 0) unit = atomicAdd(p.queue, 1u);
        unit = __builtin_amdgcn_readfirstlane(unit);
        unsigned long long first = (unsigned long long) unit * P, viewBase = 0;
        uint32_t npx;
        if constexpr (VIEWS) { // the unit's view, its pixels inside that view, the view's camera and seed key (all wave-uniform)
            if ((unsigned long long) unit >= (unsigned long long) p.n_views * p.view_units) break;
            const rtviews::Unit u = rtviews::unit_of(rtviews::Plan{p.view_pixels, P, p.n_views}, p.view_units, unit);
            first = u.first; npx = u.npx; viewBase = (unsigned long long) u.view * p.view_pixels;
            set_view<VIEWS>(pu, p, u.view);
        } else {
        if (first >= nLocal) break;
        if constexpr (JOB) { if (unit == 0xFFFFFFFFu || (job->limit >= 0 && (long long) unit >= job->limit)) break; }
        npx = (uint32_t) ((nLocal - first < (unsigned long long) P) ? (nLocal - first) : (unsigned long long) P);
        }

        // per-pixel coordinates (Scene.fs:219,226) and stream key; clear the accumulators
        for (uint32_t i = (uint32_t) lane; i < 6u * P; i += 64u) acc[i] = 0u;
        if (PASS_A && (uint32_t) lane < P) acc[10u * P + lane] = 0u;
        unsigned long long lp = 0; // local pixel of lane j < npx
        unsigned long long op = 0; // ... and where its PixelStats go: lp, in a batch of views the batch pixel
        if ((uint32_t) lane < npx) {
            lp = first + (uint32_t) lane;
            op = VIEWS ? viewBase + lp : lp;
            if constexpr (FP) footprint_setup(p, lp, pix, lane);
            else {
                uint32_t c2;
                const uint32_t c1 = pixel_setup<LDS, COUNT, D.pixels>(pu, sc, lp, pix, lane, c2);
                cand[lane * 2] = c1;
                cand[lane * 2 + 1] = c2;
            }
        }
        __builtin_amdgcn_wave_barrier();

        // ---- phase 1: 2k+1 samples per pixel, sums split after sample k (Scene.fs:172-182) ----
        run_items<LDS, COUNT, PASS_A, TEX, LOG, FP>(pu, sc, pool, poolLds, acc, pix, cand, live, false, npx * n1, n1, 0u, k + 1u, cnt, ss);
        __builtin_amdgcn_wave_barrier();

        // ---- decide (Scene.fs:177-188) and compact the pixels that continue ----
        int sumR = 0, sumG = 0, sumB = 0, count = 0;
        bool cont = false;
        if ((uint32_t) lane < npx) {
            int aR = (int) lds_take(acc + lane * 3 + 0), aG = (int) lds_take(acc + lane * 3 + 1), aB = (int) lds_take(acc + lane * 3 + 2);
            int bR = (int) lds_take(acc + P * 3 + lane * 3 + 0), bG = (int) lds_take(acc + P * 3 + lane * 3 + 1),
                bB = (int) lds_take(acc + P * 3 + lane * 3 + 2);
            int c1 = (int) k + 1;
            count = (int) n1;
            sumR = aR + bR; sumG = aG + bG; sumB = aB + bB;
            // PixelStats.mean (Pixel.fs:103-108) is integer division; Pixel.difference (Pixel.fs:113-116) is L1
            int oR = (aR / c1) & 0xFF, oG = (aG / c1) & 0xFF, oB = (aB / c1) & 0xFF;
            int nR = (sumR / count) & 0xFF, nG = (sumG / count) & 0xFF, nB = (sumB / count) & 0xFF;
            int diff = abs(nR - oR) + abs(nG - oG) + abs(nB - oB);
            if (diff == 0) earlyCount++;
            cont = (diff != 0) && (n2 > 0u);
        }
        const unsigned long long liveMask = __builtin_amdgcn_ballot_w64(cont);
        const uint32_t nLive = (uint32_t) __popcll(liveMask);
        const uint32_t pos = lane_rank(liveMask);
        if (FUSED) {
            if (cont) live[pos] = (uint32_t) lane;
        } else if (nLive > 0u) { // pass A: hand the pixel over to pass B, with its cost estimate
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(p.live_count, nLive);
            base = __builtin_amdgcn_readfirstlane(base);
            if (cont) p.pairs[base + pos] = ((unsigned long long) acc[10u * P + lane] << 32) | (unsigned long long) (uint32_t) op;
        }
        __builtin_amdgcn_wave_barrier();

        // ---- phase 2: the remaining spp-2k-1 samples of the surviving pixels (Scene.fs:191-192) ----
        if (FUSED && nLive > 0u) {
            run_items<LDS, COUNT, false, TEX, LOG, FP>(pu, sc, pool, poolLds, acc, pix, cand, live, true, nLive * n2, n2, n1, 0xFFFFFFFFu, cnt, ss);
            __builtin_amdgcn_wave_barrier();
        }

        // ---- PixelStats and mean out: one 16-byte store per pixel ----
        if ((uint32_t) lane < npx) {
            if (FUSED && cont) {
                sumR += (int) lds_take(acc + lane * 3 + 0);
                sumG += (int) lds_take(acc + lane * 3 + 1);
                sumB += (int) lds_take(acc + lane * 3 + 2);
                count += (int) n2;
            }
            sampleCount += (uint64_t) count;
            i4 out; out.x = count; out.y = sumR; out.z = sumG; out.w = sumB;
            ((i4 *) p.accum)[op] = out;
            if (p.rgb) {
                p.rgb[op * 3 + 0] = (uint8_t) (sumR / count);
                p.rgb[op * 3 + 1] = (uint8_t) (sumG / count);
                p.rgb[op * 3 + 2] = (uint8_t) (sumB / count);
            }
        }
        __builtin_amdgcn_wave_barrier();
        // a job: the unit's pixels are final (fused), or those of them that stopped early are (pass A; pass B publishes the others)
        if constexpr (JOB) { if (lane == 0) job_publish(*job, FUSED ? npx : npx - nLive); }
    }
    }

    // ---- counters: one wave reduction and a few atomics per wave per launch ----
    uint64_t e = wave_sum_u64(earlyCount), s = wave_sum_u64(sampleCount);
    if (COUNT) {
        uint64_t a = wave_sum_u64(cnt.rays), b = wave_sum_u64(cnt.aabb), c = wave_sum_u64(cnt.prim), dd = wave_sum_u64(cnt.refl);
        if (lane == 0) {
            atomicAdd(&p.counters[0], (unsigned long long) a);
            atomicAdd(&p.counters[1], (unsigned long long) b);
            atomicAdd(&p.counters[2], (unsigned long long) c);
            atomicAdd(&p.counters[3], (unsigned long long) dd);
            const unsigned long long tEnd = __builtin_amdgcn_s_memrealtime();
            atomicAdd(&p.counters[14], tEnd - tStart);                         // sum of wave lifetimes
            atomicMax(&p.counters[15], tEnd);                                  // last wave to finish
            atomicMax(&p.counters[7], 0x4000000000000000ull - tStart);         // (2^62 - earliest start)
        }
    }
    if ((COUNT || RTD_CLK) && lane == 0) {
        atomicAdd(&p.counters[8], (unsigned long long) ss.refill);
        atomicAdd(&p.counters[9], (unsigned long long) ss.trips);
        atomicAdd(&p.counters[10], (unsigned long long) ss.leaf);
        atomicAdd(&p.counters[11], (unsigned long long) ss.shade);
        atomicAdd(&p.counters[12], (unsigned long long) ss.refillLanes);
        atomicAdd(&p.counters[13], (unsigned long long) ss.shadeLanes);
        atomicAdd(&p.counters[20], (unsigned long long) ss.slow);
        atomicAdd(&p.counters[21], (unsigned long long) ss.slowLanes);
        atomicAdd(&p.counters[22], (unsigned long long) ss.parkedLanes);
        atomicAdd(&p.counters[23], ss.tRefill);
        atomicAdd(&p.counters[24], ss.tSlow);
        atomicAdd(&p.counters[25], ss.tWalk);
        atomicAdd(&p.counters[26], ss.tShade);
        if (RTD_CLK) {
            atomicAdd(&p.counters[27], ss.tLoop);
            atomicAdd(&p.counters[28], ss.tLeaf);
            atomicAdd(&p.counters[29], ss.tUnb);
            atomicAdd(&p.counters[30], ss.tCam);
            atomicAdd(&p.counters[31], ss.tLamb);
            if (!COUNT) { atomicAdd(&p.counters[14], ss.loopTrips); atomicAdd(&p.counters[15], ss.loopLanes); } // (the counting variant keeps its wave lifetimes there)
#ifdef RTD_STAGE_CLOCKS
            if (!COUNT && PASS_B) { // the census describes pass B's timed kernel
                const uint32_t cz[16] = {ss.turns, ss.lambBatches, ss.lambLanes, ss.newRefills, ss.newItems, ss.unparkL, ss.unparkA, ss.storeBlocksL, ss.storeLanesL,
                                         ss.storeBlocksA, ss.lightBatches, ss.lightLanes, ss.missLanes, ss.ranges, ss.flushes, ss.leafLanes};
                for (int i = 0; i < 16; ++i) atomicAdd(&g_census[i], (unsigned long long) cz[i]);
                for (int i = 0; i < 8; ++i) { atomicAdd(&g_census[16 + i], (unsigned long long) ss.slowLanesByStyle[i]); atomicAdd(&g_census[24 + i], (unsigned long long) ss.slowBatchesByStyle[i]); }
                // the stage counts of rt_last_stage_stats, for this kernel alone (those sum pass A and pass B)
                const unsigned long long sz[12] = {ss.refill, ss.trips, ss.leaf, ss.shade, ss.refillLanes, ss.shadeLanes, ss.slow, ss.slowLanes, ss.loopTrips, ss.loopLanes,
                                                   ss.unparkBatchesL, ss.unparkBatchesA};
                for (int i = 0; i < 12; ++i) atomicAdd(&g_census[36 + i], sz[i]);
            }
#endif
        }
    }
    if (lane == 0) {
        atomicAdd(&p.counters[4], (unsigned long long) s);
        atomicAdd(&p.counters[5], (unsigned long long) e);
    }
