"""Every launching Scene method, its tensor route against its array route, bit for bit, at the smallest shapes where a wrapper can go
wrong: the 9x7 frame of tests/test_refusal_messages.py, lists of 0, 1 and 65 entries (frame shards of 0, 1 and 7 rows), every input
that may be non-contiguous passed as a strided view.  The two routes share one body per method, so this holds the shared body to both
entry points of each pair; stats=False (tensor route: no wait, no statistics) must leave last_stats None and write the same buffers.
What the methods compute is the business of the test_gpu_* file of each."""
import dataclasses

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

MAX_W, MAX_H = 4, 3
COLS, ROWS = 2 * MAX_W + 1, 2 * MAX_H + 1
FRAME = COLS * ROWS
F = (MAX_W, MAX_H)
SEED, DEPTH, DONE, SPP = 5, 6, 12, 20


@dataclasses.dataclass
class World:
    scene: object
    cam: dict  # samples per pixel -> camera


@pytest.fixture(scope="module")
def world(rt):
    objs, _, _, _ = scenes.all_materials()
    cam = {spp: dataclasses.replace(rt.Camera.makeBasic(spp, 1.0, COLS / ROWS, scenes.P(0.0, 0.3, -1.0), scenes.unit(0.0, -0.05, 1.0),
                                                        scenes.V(0.0, 1.0, 0.0)), BounceDepth=DEPTH) for spp in (DONE, SPP)}
    return World(rt.Scene.make(objs), cam)


def strided(a):
    """The same values as a view of every other element of the last axis."""
    return np.repeat(a, 2, axis=-1)[..., ::2]


def gpu(key, a):
    """An input on the GPU, strided if the array is and the tensor route takes it so (it extends accum in place and reads targets as they lie)."""
    import torch
    if key in ("accum", "targets") or a.flags.c_contiguous:
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return torch.from_numpy(np.repeat(a, 2, axis=-1)).cuda()[..., ::2]


def rays_of(n):
    return strided(scenes.random_rays(n, seed=3))


def states_of(n):
    return strided(np.random.default_rng(4).integers(1, 2**32, size=(n, 4), dtype=np.uint32))


def footprints_of(n):
    rng = np.random.default_rng(6)
    f = np.zeros((n, 12))
    f[:, 0:3] = (0.0, 0.3, -1.0)
    f[:, 3:6] = rng.uniform(-0.5, 0.5, size=(n, 3)) + (0.0, 0.0, 1.0)
    f[:, 6] = f[:, 10] = 0.05
    return strided(f)


def pixels_of(n):
    return strided(((np.arange(n) * 11) % FRAME).astype(np.int32))


def targets_of(shape):
    return strided((DONE + np.arange(int(np.prod(shape))) % (SPP - DONE + 1)).astype(np.int32).reshape(shape))


# method -> (its inputs for a size n, the call).  w: the World, v: the inputs on one route, kw: stats= where given
CASES = {
    "hitObject": (lambda w, n: dict(rays=rays_of(n)), lambda w, v, kw: w.scene.hitObject(v["rays"], **kw)),
    "traceRays": (lambda w, n: dict(rays=rays_of(n), rng=states_of(n)), lambda w, v, kw: w.scene.traceRays(v["rays"], DEPTH, rng=v["rng"], **kw)),
    "traceRays without rng": (lambda w, n: dict(rays=rays_of(n)), lambda w, v, kw: w.scene.traceRays(v["rays"], DEPTH, seed=SEED, stream_base=7, **kw)),
    "renderFootprints": (lambda w, n: dict(fp=footprints_of(n)), lambda w, v, kw: w.scene.renderFootprints(v["fp"], SPP, DEPTH, seed=SEED, **kw)),
    "renderFootprints extend": (
        lambda w, n: dict(fp=footprints_of(n), accum=w.scene.renderFootprints(footprints_of(n), DONE, DEPTH, seed=SEED).accum),
        lambda w, v, kw: w.scene.renderFootprints(v["fp"], SPP, DEPTH, seed=SEED, extend=(v["accum"], DONE), **kw)),
    "renderFootprints extend_map": (
        lambda w, n: dict(fp=footprints_of(n), accum=w.scene.renderFootprints(footprints_of(n), DONE, DEPTH, seed=SEED).accum, targets=targets_of((n,))),
        lambda w, v, kw: w.scene.renderFootprints(v["fp"], SPP, DEPTH, seed=SEED, extend_map=(v["accum"], v["targets"]), **kw)),
    "renderPixels": (lambda w, n: dict(px=pixels_of(n)), lambda w, v, kw: w.scene.renderPixels(*F, w.cam[SPP], v["px"], seed=SEED, **kw)),
    "renderPixels extend": (
        lambda w, n: dict(px=pixels_of(n), accum=w.scene.renderPixels(*F, w.cam[DONE], pixels_of(n), seed=SEED).accum),
        lambda w, v, kw: w.scene.renderPixels(*F, w.cam[SPP], v["px"], seed=SEED, extend=(v["accum"], DONE), **kw)),
    "cameraHits": (lambda w, n: dict(px=pixels_of(n)), lambda w, v, kw: w.scene.cameraHits(*F, w.cam[SPP], v["px"], sample_first=1, n_samples=2, seed=SEED, **kw)),
    "cameraPaths": (lambda w, n: dict(px=pixels_of(n)),
                    lambda w, v, kw: w.scene.cameraPaths(*F, w.cam[SPP], v["px"], sample_first=1, n_samples=2, max_vertices=3, summary=True, seed=SEED, **kw)),
    "tracePaths": (lambda w, n: dict(rays=rays_of(n), rng=states_of(n)),
                   lambda w, v, kw: w.scene.tracePaths(v["rays"], DEPTH, rng=v["rng"], max_vertices=3, **kw)),
}
# the frame extensions: n is a number of rows
FRAME_CASES = {
    "extend_rows": (lambda w, n: dict(accum=strided(w.scene.render_rows(*F, w.cam[DONE], seed=SEED, n_rows=n).accum)),
                    lambda w, v, kw: w.scene.extend_rows(*F, w.cam[SPP], v["accum"], DONE, seed=SEED, **kw)),
    "extend_rows_map": (lambda w, n: dict(accum=strided(w.scene.render_rows(*F, w.cam[DONE], seed=SEED, n_rows=n).accum), targets=targets_of((n, COLS))),
                        lambda w, v, kw: w.scene.extend_rows_map(*F, w.cam[SPP], v["accum"], v["targets"], seed=SEED, **kw)),
}


def buffers(result):
    """The bytes of every array or tensor of a result, in order (None where a field is None; the statistics are left out)."""
    out = []
    for x in result:
        if x is None or isinstance(x, dict):
            continue
        out.append((tuple(x.shape), (x if isinstance(x, np.ndarray) else x.cpu().numpy()).tobytes()))
    return out


# An empty tensor has no address (its data_ptr() is 0) and the path calls refuse a call all of whose outputs are absent, so the tensor route
# of an empty list is refused by the library where the array route returns empty arrays.  That is how the routes have always differed.
EMPTY_TENSORS_REFUSED = ("cameraPaths", "tracePaths")


def _compare(rt, world, method, inputs, call, sizes):
    import torch
    for n in sizes:
        v = inputs(world, n)
        want = buffers(call(world, v, {}))
        assert isinstance(world.scene.last_stats, dict)
        assert want and all(shape[0] == n for shape, _ in want), n
        if n == 0 and method in EMPTY_TENSORS_REFUSED:
            with pytest.raises(rt.RtError, match="every output is NULL"):
                call(world, {k: gpu(k, a) for k, a in v.items()}, {})
            continue
        got = call(world, {k: gpu(k, a) for k, a in v.items()}, {})
        assert all(x is None or isinstance(x, dict) or x.is_cuda for x in got)
        assert buffers(got) == want, n
        assert isinstance(world.scene.last_stats, dict) and all(x == world.scene.last_stats for x in got if isinstance(x, dict))
    quiet = call(world, {k: gpu(k, a) for k, a in v.items()}, dict(stats=False))  # the largest size once more, without a wait
    assert world.scene.last_stats is None and not any(isinstance(x, dict) for x in quiet)
    torch.cuda.synchronize()
    assert buffers(quiet) == want


@pytest.mark.parametrize("method", list(CASES))
def test_the_tensor_route_equals_the_array_route_for_lists(rt, world, method):
    _compare(rt, world, method, *CASES[method], sizes=(0, 1, 65))


@pytest.mark.parametrize("method", list(FRAME_CASES))
def test_the_tensor_route_equals_the_array_route_for_frame_shards(rt, world, method):
    _compare(rt, world, method, *FRAME_CASES[method], sizes=(0, 1, ROWS))


@pytest.mark.parametrize("method", ["cameraHits", "cameraPaths"])
def test_the_frames_first_pixels_without_a_list_on_both_routes(rt, world, method):
    import torch
    call = getattr(world.scene, method)
    for n in (0, 1, None):  # None: the whole frame
        want = buffers(call(*F, world.cam[SPP], n=n, n_samples=2, seed=SEED))
        assert want[0][0][0] == (FRAME if n is None else n)
        if n == 0 and method in EMPTY_TENSORS_REFUSED:
            with pytest.raises(rt.RtError, match="every output is NULL"):
                call(*F, world.cam[SPP], n=n, n_samples=2, seed=SEED, tensors=True)
            continue
        assert buffers(call(*F, world.cam[SPP], n=n, n_samples=2, seed=SEED, tensors=True)) == want
    quiet = call(*F, world.cam[SPP], n_samples=2, seed=SEED, tensors=True, device=torch.cuda.current_device(), stats=False)
    assert world.scene.last_stats is None and quiet.stats is None
    torch.cuda.synchronize()
    assert buffers(quiet) == want
