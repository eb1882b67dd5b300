"""GPU, 2 ranks sharing cuda:0 over gloo: SlabFrame.construct_graph on two slabs gives the one-rank node list (the band samples
are gathered over ranks and ordered canonically before the subsampling), with either sampler."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, ws, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        from dynamicfusion_body_amd import graph, scene
        from dynamicfusion_body_amd.pipeline import SlabFrame
        torch.cuda.set_device(0)
        R, radius = 64, 5.0
        H, W, fx, cx, cy = scene.CAMERAS["C1"]
        K = scene.intrinsics(fx, cx, cy)
        scale, center, tdist = scene.grid_params(R)
        lws = [scene.view_extrinsic(a) for a in (0.0, 40.0)]
        depths = [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda() for lw in lws]

        def frame(distributed):
            sf = SlabFrame(K, scale, center, R, tdist / scale, None, None, knn=4, pcg_iters=10, band=2.0, distributed=distributed)
            for d, lw in zip(depths, lws):
                sf.integrate(d, lw)
            return sf
        whole = frame(False)                                            # this process alone, the whole grid
        n_whole = whole.construct_graph(radius)
        want = whole.fs.solver.node_pos.cpu().numpy()
        pts = whole.band_samples()[0].cpu().numpy()
        host, _ = graph.uniform_sample(pts[np.lexsort((pts[:, 2], pts[:, 1], pts[:, 0]))], radius)
        assert n_whole > 20 and np.array_equal(want, host)
        for sampler in ("device", "host"):
            slab = frame(True)                                          # one of two slabs
            assert slab.ws == ws and slab.b - slab.a == R // ws
            assert 0 < slab.band_samples()[0].shape[0] < len(pts)
            assert slab.construct_graph(radius, sampler=sampler) == n_whole
            assert np.array_equal(slab.fs.solver.node_pos.cpu().numpy(), want), sampler
        out[rank] = 1
    finally:
        dist.destroy_process_group()


def test_two_ranks_build_the_one_rank_graph():
    ws = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    out = ctx.Array("i", [0] * ws)
    procs = [ctx.Process(target=_worker, args=(r, ws, port, out)) for r in range(ws)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
    for p in procs:
        if p.is_alive():                                                # (a rank that waits for a peer that has failed)
            p.kill()
    assert all(p.exitcode == 0 for p in procs)
    assert list(out) == [1] * ws
