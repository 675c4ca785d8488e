"""A 360-degree equirectangular panorama of a catalogue scene: an example of a camera the render kernel does not have, rendered
in ONE call through Scene.renderFootprints, and a measurement aid for the footprint and ray-list modes.

Footprints are built with torch on the GPU, one per pixel, from the scene camera's eye: base is the direction of the pixel's corner,
du and dv the direction differences to the next column and row, so the samples jitter inside the pixel; sample s of pixel p draws
from the stream keyed (seed, p, s), and the adaptive stop is Scene.renderPixel's.  The image goes out through ImageOutput.writePpm.
--legacy-loop renders as this script did before footprints existed: one ray per pixel (through its centre), spp Scene.traceRays
launches, the colours summed in torch and divided as PixelStats.mean does -- no jitter, no adaptive stop.
--measure N times both (and the footprint path with du = dv = 0 through the pixel centres, the like-for-like workload), N times each,
alternating in this process after a warm-up, and prints kernel and wall times.
--compare also times Scene.hitObject, the one-thread-per-ray rt_dev_trace_ray / rt_dev_hit_object hooks on the same rays, and
Scene.traceRays / hitObject on random rays through the scene.

usage: python scripts/panorama.py [--scene random-spheres] [--width 1024] [--spp 16] [--depth 50] [--out pano.ppm] [--legacy-loop]
                                  [--measure N] [--compare]"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ray_tracing_fsharp_amd as rt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default="random-spheres", help="a name of sample_images.CATALOGUE (random-spheres: the bench's config-3 scene)")
ap.add_argument("--width", type=int, default=1024, help="panorama width in pixels; the height is half of it")
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--depth", type=int, default=50)
ap.add_argument("--seed", type=int, default=2024)
ap.add_argument("--out", default="panorama.ppm")
ap.add_argument("--compare", action="store_true", help="also time hitObject, the rt_dev_* hooks and random rays")
ap.add_argument("--legacy-loop", action="store_true", help="spp traceRays launches summed in torch instead of one renderFootprints call")
ap.add_argument("--measure", type=int, default=0, metavar="N", help="time the legacy loop, renderFootprints and renderFootprints with du = dv = 0, N times each")
a = ap.parse_args()

objs, cam = rt.sample_images.get(a.scene)()[:2]
scene = rt.Scene.make(objs)
eye = torch.tensor(list(cam.abi.view_origin), dtype=torch.float64, device="cuda")
W, H = a.width, a.width // 2
# equirectangular: column -> longitude in [-pi, pi), row -> latitude from +pi/2 (top) to -pi/2; y is up



def direction(row, col):
    lo_ = col * (2.0 * math.pi / W) - math.pi
    la_ = 0.5 * math.pi - row * (math.pi / H)
    return torch.stack([torch.cos(la_) * torch.sin(lo_), torch.sin(la_), torch.cos(la_) * torch.cos(lo_)], dim=-1).reshape(-1, 3)


d = direction(*torch.meshgrid(torch.arange(H, dtype=torch.float64, device="cuda") + 0.5, torch.arange(W, dtype=torch.float64, device="cuda") + 0.5, indexing="ij"))
rays = torch.cat([eye.expand(d.shape[0], 3), d], dim=1).contiguous()  # through the pixel centres (the legacy loop, --compare)
n = rays.shape[0]
rr, cc = torch.meshgrid(torch.arange(H, dtype=torch.float64, device="cuda"), torch.arange(W, dtype=torch.float64, device="cuda"), indexing="ij")
corner = direction(rr, cc)
footprints = torch.cat([eye.expand(n, 3), corner, direction(rr, cc + 1.0) - corner, direction(rr + 1.0, cc) - corner], dim=1).contiguous()
centres = torch.cat([rays, torch.zeros((n, 6), dtype=torch.float64, device="cuda")], dim=1).contiguous()  # du = dv = 0: the legacy loop's rays


def legacy_loop():
    """-> (mean rgb [n, 3] uint8, samples, summed kernel_ms, wall ms)"""
    sums = torch.zeros((n, 3), dtype=torch.int32, device="cuda")  # PixelStats sums: Count is spp for every pixel
    kernel_ms = 0.0
    t0 = time.perf_counter()
    for s in range(a.spp):
        colour, _ = scene.traceRays(rays, a.depth, seed=a.seed, stream_base=0, sample=s)
        kernel_ms += scene.last_stats["kernel_ms"]
        sums += colour.to(torch.int32)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return torch.div(sums, a.spp, rounding_mode="floor").to(torch.uint8), n * a.spp, kernel_ms, wall * 1e3  # PixelStats.mean: integer division


def one_call(fp, counters=False):
    t0 = time.perf_counter()
    res = scene.renderFootprints(fp, a.spp, a.depth, seed=a.seed, counters=counters)
    torch.cuda.synchronize()
    return res.rgb, res.stats["samples"], res.stats["kernel_ms"], (time.perf_counter() - t0) * 1e3


mean, paths, kernel_ms, wall = legacy_loop() if a.legacy_loop else one_call(footprints)
rt.ImageOutput.writePpm(False, lambda _: None, mean.reshape(H, W, 3).cpu().numpy(), a.out)
print(f"panorama {W}x{H} of {a.scene}, {a.spp} spp, depth {a.depth} ({'legacy loop' if a.legacy_loop else 'renderFootprints'}): {paths} paths in "
      f"{kernel_ms:.1f} ms of kernels ({paths / kernel_ms / 1e3:.1f} M paths/s; wall {wall:.1f} ms) -> {a.out}")
if a.legacy_loop:
    _, _ = scene.traceRays(rays, a.depth, seed=a.seed, counters=True)
    per = scene.last_stats["rays"] / n
else:
    st = scene.renderFootprints(footprints, a.spp, a.depth, seed=a.seed, counters=True).stats
    per = st["rays"] / st["samples"]
    print(f"  {st['pixels_early']} of {st['pixels']} pixels stop early")
print(f"  rays per path (counting variant): {per:.2f} -> {paths * per / kernel_ms / 1e3:.1f} M rays/s")

if a.measure:
    for label, fp in (("renderFootprints, jittered", footprints), ("renderFootprints, du = dv = 0", centres)):
        st = scene.renderFootprints(fp, a.spp, a.depth, seed=a.seed, counters=True).stats  # (also the warm-up of the counting kernels)
        print(f"measure: {label}: {st['samples']} samples, {st['rays']} rays, {st['pixels_early']} of {st['pixels']} pixels stop early")
    legacy_loop(), one_call(footprints), one_call(centres)  # warm-up
    for i in range(a.measure):
        for label, fn in (("legacy loop", legacy_loop), ("renderFootprints, jittered", lambda: one_call(footprints)),
                          ("renderFootprints, du = dv = 0", lambda: one_call(centres))):
            _, smp, kms, w = fn()
            print(f"measure {i}: {label}: {smp} samples, kernels {kms:.2f} ms, wall {w:.2f} ms, {smp / kms / 1e3:.1f} M paths/s of kernel time")

if a.compare:
    def timed(fn, reps=3):
        best = float("inf")
        for _ in range(reps):
            t = time.perf_counter()
            out = fn()
            best = min(best, time.perf_counter() - t)
        return best * 1e3, out

    def report(label, rr):
        host = rr.cpu().numpy()
        m = len(host)
        g = np.random.default_rng(1).integers(1, 2**31, size=(m, 4), dtype=np.uint32)
        unit = host.copy()
        unit[:, 3:] /= np.linalg.norm(unit[:, 3:], axis=1, keepdims=True)  # the hooks take Ray.make's result
        ms_t = min((scene.traceRays(rr, a.depth, rng=torch.from_numpy(g).cuda()), scene.last_stats["kernel_ms"])[1] for _ in range(3))
        wall_t, _ = timed(lambda: scene.traceRays(host, a.depth, rng=g))
        ms_h = min((scene.hitObject(rr), scene.last_stats["kernel_ms"])[1] for _ in range(3))
        wall_h, _ = timed(lambda: scene.hitObject(host))
        hook_t, _ = timed(lambda: rt.hooks.trace_ray(scene, a.depth, unit, g))
        hook_h, _ = timed(lambda: rt.hooks.hit_object(scene, unit))
        print(f"{label}: {m} rays")
        print(f"  traceRays  kernel {ms_t:8.2f} ms ({m / ms_t / 1e3:7.1f} M paths/s)  host call {wall_t:8.2f} ms | "
              f"rt_dev_trace_ray host call {hook_t:8.2f} ms: {hook_t / wall_t:.1f}x")
        print(f"  hitObject  kernel {ms_h:8.2f} ms ({m / ms_h / 1e3:7.1f} M rays/s)   host call {wall_h:8.2f} ms | "
              f"rt_dev_hit_object host call {hook_h:8.2f} ms: {hook_h / wall_h:.1f}x")

    report("panorama rays", rays)
    gen = torch.Generator(device="cuda").manual_seed(5)
    m = 1 << 20
    o = torch.randn((m, 3), dtype=torch.float64, device="cuda", generator=gen) * 4.0 + torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device="cuda")
    v = torch.randn((m, 3), dtype=torch.float64, device="cuda", generator=gen)
    report("random rays", torch.cat([o, v], dim=1).contiguous())
