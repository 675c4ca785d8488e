"""BASELINE config 4 (the final scene at maxW=3840, maxH=2160 -> 7681x4321 px, 1000 spp) on one GPU, and the real two-rank path
(HIP renderer in every rank, torch.distributed gather) with both ranks on this box's one GPU."""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config4_full_frame_properties_rows_and_shard(rt, orc):
    """33.2 Mpx x 1000 spp, 6.0e10 rays, ~3.3 s: size-independent properties on the whole frame (Count is 11 or 1000, sums bounded,
    samples = sum of Counts, sky rows are the dome colour exactly, counters are those
    of the committed run), three image rows against the oracle, and rank 3's 1-of-8 interleaved shard equal to the same rows of
    the frame."""
    objs, cam, _, _ = rt.sample_images.config3_final(seed=2024, spp=1000, depth=50)
    w, h = 3840, 2160
    s = rt.Scene.make(objs)
    a = s.render_rows(w, h, cam, seed=2024, counters=True)
    assert a.accum.shape == (4321, 7681, 4)
    cnt = a.accum[..., 0]
    assert set(np.unique(cnt)) <= {11, 1000}
    assert np.all(a.accum[..., 1:] >= 0) and np.all(a.accum[..., 1:] <= 255 * cnt[..., None])
    assert a.stats["samples"] == int(cnt.sum(dtype=np.int64)) and a.stats["pixels_early"] == int((cnt == 11).sum())
    assert np.all(a.accum[0, :, 0] == 11) and np.all(a.accum[0, :, 1:] == np.array([200, 200, 255]) * 11)
    # the dome encloses everything, but 1 ray of the 6.0e10 finds no positive root on it (both roots inside the 1e-8 band): Black, as in the reference
    assert 0 <= a.stats["rays"] - a.stats["reflections"] <= 2 and a.stats["pixels"] == 4321 * 7681
    assert (a.stats["rays"], a.stats["prim_tests"], a.stats["samples"]) == CONFIG4_COUNTERS, (a.stats["rays"], a.stats["prim_tests"], a.stats["samples"])
    o = orc.OracleScene(objs)
    for row in (300, 1730, 2700):  # sky, horizon, spheres
        acc, rgb, st = o.render_rows(w, h, cam.to_abi(), seed=2024, row_first=row, row_stride=1, n_rows=1, threads=16)
        assert np.array_equal(a.accum[row], acc[0]) and np.array_equal(a.rgb[row], rgb[0]), row
    part = s.render_rows(w, h, cam, seed=2024, row_first=3, row_stride=8, counters=True)
    assert np.array_equal(part.accum, a.accum[3::8]) and part.stats["samples"] == int(cnt[3::8].sum(dtype=np.int64))
    # the kernel that is timed (no counters): the same frame, every PixelStats
    timed = s.render_rows(w, h, cam, seed=2024)
    assert np.array_equal(timed.accum, a.accum) and np.array_equal(timed.rgb, a.rgb)


CONFIG4_COUNTERS = (59957428074, 196481361316, 18394792971)  # rays, leaf + unbounded tests, samples: deterministic in the seed


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist

    import ray_tracing_fsharp_amd as rt
    import scenes
    from ray_tracing_fsharp_amd import distributed as rtd

    torch.cuda.set_device(0)  # one GPU on this box: every rank renders on it; gloo stages the gather through host memory
    dist.init_process_group("gloo", rank=rank, world_size=world)
    objs, cam, w, h = scenes.small_final(spp=40, pixels=30)  # 61 rows: ragged shards
    scene = rt.Scene.make(objs)
    rows, cols = 2 * h + 1, 2 * w + 1
    first, stride, n = rtd.shard_rows(rows, rank, world)
    local = torch.zeros(((rows + world - 1) // world, cols, 4), dtype=torch.int32, device="cuda:0")
    st = rtd.render_shard_device(scene, cam, w, h, 33, 0, first, stride, n, local, stream=torch.cuda.current_stream().cuda_stream,
                                 counters=True, want_stats=True)
    frame = rtd.gather_frame(local, rows, cols, rank, world)
    tot = torch.tensor([float(st[k]) for k in ("rays", "prim_tests", "reflections", "samples", "pixels_early")], dtype=torch.float64)
    dist.all_reduce(tot)
    if rank == 0:
        np.savez(out_path, frame=frame.cpu().numpy(), totals=tot.numpy())
    else:
        assert frame is None
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_two_ranks_with_the_hip_renderer_equal_one_rank(rt, tmp_path, world):
    """bench.py's N > 1 path with the product renderer in every rank (not the oracle stand-in of the CPU test): shard_rows ->
    rt_render_device into a padded CUDA tensor -> one gather -> de-interleave, against the single-rank frame and job counters."""
    import torch.multiprocessing as mp

    import scenes

    out = str(tmp_path / "frame.npz")
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    got = np.load(out)
    objs, cam, w, h = scenes.small_final(spp=40, pixels=30)
    one = rt.Scene.make(objs).render_rows(w, h, cam, seed=33, counters=True)
    assert np.array_equal(got["frame"], one.accum)
    assert [int(x) for x in got["totals"]] == [one.stats[k] for k in ("rays", "prim_tests", "reflections", "samples", "pixels_early")]
