"""A 360-degree equirectangular panorama of a catalogue scene through Scene.traceRays: an example of a camera the render kernel
does not have, and a measurement aid for the ray-list mode.

Camera rays are built with torch on the GPU (one per pixel, from the scene camera's eye); sample s of pixel p draws from the stream
keyed (seed, stream_base = p, sample = s), as a render's sample would.  The spp samples are averaged as PixelStats does (integer
sums, integer mean) and the image goes out through ImageOutput.writePpm.  Prints paths/s from the kernels' own time (kernel_ms).
--compare also times Scene.hitObject, the one-thread-per-ray rt_dev_trace_ray / rt_dev_hit_object hooks on the same rays, and
Scene.traceRays / hitObject on random rays through the scene.

usage: python scripts/panorama.py [--scene random-spheres] [--width 1024] [--spp 16] [--depth 50] [--out pano.ppm] [--compare]"""
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
a = ap.parse_args()

objs, cam = rt.sample_images.get(a.scene)()[:2]
scene = rt.Scene.make(objs)
eye = torch.tensor(list(cam.abi.view_origin), dtype=torch.float64, device="cuda")
W, H = a.width, a.width // 2
# equirectangular: column -> longitude in [-pi, pi), row -> latitude from +pi/2 (top) to -pi/2; y is up
lon = (torch.arange(W, dtype=torch.float64, device="cuda") + 0.5) * (2.0 * math.pi / W) - math.pi
lat = 0.5 * math.pi - (torch.arange(H, dtype=torch.float64, device="cuda") + 0.5) * (math.pi / H)
la, lo = torch.meshgrid(lat, lon, indexing="ij")
d = torch.stack([torch.cos(la) * torch.sin(lo), torch.sin(la), torch.cos(la) * torch.cos(lo)], dim=-1).reshape(-1, 3)
rays = torch.cat([eye.expand(d.shape[0], 3), d], dim=1).contiguous()
n = rays.shape[0]

sums = torch.zeros((n, 3), dtype=torch.int32, device="cuda")  # PixelStats sums: Count is spp for every pixel
kernel_ms = 0.0
t0 = time.perf_counter()
for s in range(a.spp):
    colour, _ = scene.traceRays(rays, a.depth, seed=a.seed, stream_base=0, sample=s)
    kernel_ms += scene.last_stats["kernel_ms"]
    sums += colour.to(torch.int32)
torch.cuda.synchronize()
wall = time.perf_counter() - t0
mean = torch.div(sums, a.spp, rounding_mode="floor").to(torch.uint8)  # PixelStats.mean (Pixel.fs:103-108): integer division
rt.ImageOutput.writePpm(False, lambda _: None, mean.reshape(H, W, 3).cpu().numpy(), a.out)
paths = n * a.spp
print(f"panorama {W}x{H} of {a.scene}, {a.spp} spp, depth {a.depth}: {paths} paths in {kernel_ms:.1f} ms of kernels "
      f"({paths / kernel_ms / 1e3:.1f} M paths/s; wall {wall * 1e3:.1f} ms) -> {a.out}")
_, _ = scene.traceRays(rays, a.depth, seed=a.seed, counters=True)
per = scene.last_stats["rays"] / n
print(f"  rays per path (counting variant): {per:.2f} -> {paths * per / kernel_ms / 1e3:.1f} M rays/s")

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
