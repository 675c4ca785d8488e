// rt_launch_consts.h -- the constants the launch planner (rt_launch_plan.h) shares with the device code.  Nothing but #defines, so
// that a plain C++ compiler reads it; rt_device.h includes it for the kernels.  The measurements in the comments are the record of
// how each value was chosen.
#pragma once

// ---- work units and the waves' LDS scratch (rt_render_kernel.h) ----
#define RTD_MAX_CHUNK 64
#define RTD_MAX_PARK 256
#define RTD_PARK_DEFAULT 96 /* entries of a wave's general pool (88 B each, global memory).  Bench frame, ms / GB written to HBM: 45: 124.6, 64: 109.7 / 14.5, 80: 108.8 / 24.0, 96: 108.2 / 28.1, 128: 108.2 / 30.7 (scripts/pool_traffic.sh) */
#ifndef RTD_PARK_L_DEFAULT
#define RTD_HYBRID_LANES 16 /* node_loop_glb32: this many lanes at LDS-held records make a trip of their own (measured, rt_device.h) */
#define RTD_PARK_L_DEFAULT 64 /* entries of a wave's pool of parked Lambert hits; 0: Lambert hits are shaded where they fall */
#endif
// Per-wave LDS scratch in 4-byte words, P = pixels per work unit (layout: rt_render_kernel.h)
#define RTD_WAVE_WORDS(P) (18u * (uint32_t) (P)) /* fused: 13 P used; pass B: two slots of {acc [P][3], pix [P][4]}, then cand [2][P][2] */
#define RTD_WAVE_WORDS_A(P) (13u * (uint32_t) (P)) /* pass A: acc, pix, cost, cand [P][2] -- a tighter footprint, so its units can be wider */
#define RTD_WAVE_WORDS_MAP(P) (22u * (uint32_t) (P)) /* pass B of an extension by map: pass B's 18 P, then per slot first item [P] and sample base [P] */
#define RTD_WAVE_WORDS_CAM(P) (6u * (uint32_t) (P)) /* camera hits: pix [P][4] and cand [P][2] of the unit being handed out; nothing is accumulated */

// ---- the lane scheduler's thresholds (rt_render_kernel.h, Sched) ----
#define RTD_YIELD_DEFAULT 50
#define RTD_LEAF_WAIT_EXTRA 5 /* RenderParams::leaf_wait = yield_lanes + this (at most 64) */
#define RTD_REFILL_DEFAULT 8

// ---- parked paths ----
#define RTD_PARK_ENTRY_BYTES 96 /* 5 x 16 B + 8 B, padded */
#define RTD_PARK_L_LDS_BYTES 56 /* a parked Lambert hit in LDS: strike 24, rng 16, colour, slot, bounces | inside << 31, object */

// ---- pass B's cost-ordered list: bucket sort of (cost, pixel) pairs ----
#define RTD_COST_BUCKETS 64

// ---- extending a rendered buffer (rt_render_extend; DESIGN.md "Extending a frame") ----
#define RTD_EARLY_COUNT 11     /* PixelStats.Count of a pixel that stopped early at any spp >= 10: 2k+1 with k = min 5 (spp/2) = 5 */
#define RTD_EXTEND_MIN_DONE 12 /* the least samples_done: k is 5 on both sides, and Count tells a stopped pixel (11) from a finished one */

// ---- scene image (rt_device.h) ----
#define RTD_NODE32_BYTES 64 /* a single-precision filter record of the timed node loop */

// ---- the output stage (rt_output.h; DESIGN.md "Output on the device") ----
#define RTO_BLOCK 256           /* threads of a tile's workgroup */
#define RTO_THREAD_PIXELS 4     /* consecutive pixels per thread: 12 colour bytes */
#define RTO_TILE_PIXELS (RTO_BLOCK * RTO_THREAD_PIXELS) /* 1024 pixels: 3 KiB of colour in, at most 12 KiB of P3 text (25 KiB of pixel map) staged in LDS */
#define RTO_PPM_PIXEL_BYTES 12  /* "255 255 255" and one separator */
#define RTO_MAP_PIXEL_BYTES 25  /* ten digits, ',', ten digits, '\n', three colour bytes */
#define RTO_SCAN_THREADS 1024   /* tile sums per trip of the one scanning workgroup: trips begin at RTO_SCAN_THREADS * RTO_TILE_PIXELS = 2^20 pixels */
#define RTO_SCRATCH_HEAD 16     /* struct FormatScratch; one uint64 per tile follows */
#define RTO_PNG_TILE_BYTES 16384 /* filtered bytes of a PNG tile = one deflate block (rt_png.h): 64 per thread; 16 KiB staged in, at most 16 KiB + 5 out */

// ---- host side ----
// LDS budget: 160 KiB per CU (MI355X_MICROARCH.md); the LDS part of the scene image plus every wave's scratch must fit one workgroup.
#define RT_LDS_BYTES 163840u
// Per-launch scratch, stream-ordered (hipMallocAsync on the launch stream): struct LaunchScratch (rtfs_amd.hip).  Nothing is
// shared between launches, so any number of them may be in flight on any streams.
#define RT_SCRATCH_BYTES 512
