"""The code Fusion and FusionDM share (canonical.CanonicalModel), checked on both classes against the layer below it: each
method must do what calling mesh.* / kernels.* / pipeline.* directly does.  16^3 volume: a sphere of radius 5 voxels and a
detached two-voxel blob; 24 x 32 depth maps of scene.py's sphere."""
import os
import re

import numpy as np
import pytest
import torch

from dynamicfusion_body_amd import Fusion, FusionDM, kernels, mesh, scene
from dynamicfusion_body_amd.pipeline import extract_surface_samples

pytestmark = pytest.mark.gpu

R, H, W = 16, 24, 32
SCALE, CENTER, TDIST = scene.grid_params(R)                    # 0.1 m voxels around the scene's sphere: its radius is 5 voxels
K = scene.intrinsics(30.03113, 15.97033, 11.96003)             # camera C1 at a tenth of its resolution
LWS = [scene.view_extrinsic(a) for a in (0.0, 40.0)]
BOTH = pytest.mark.parametrize("cls", [Fusion, FusionDM])


def volume():
    i = np.arange(R) - (R - 1) / 2.0
    r = np.sqrt(i[:, None, None] ** 2 + i[None, :, None] ** 2 + i[None, None, :] ** 2)
    T = np.clip((r - 5.0) * SCALE, -TDIST, TDIST)
    T[1, 1, 1:3] = -0.5 * TDIST                                # the blob: a component of a few faces
    return T.astype(np.float32)


def half_weights():
    w = np.zeros((R, R, R), dtype=np.float32)
    w[:, :9] = 2.0
    return w


def depth_maps():
    return [scene.render_depth(K, lw, H, W, dtype=np.float32, wall_z=None) for lw in LWS]


def make(cls, weights=None):
    """An object of either class whose canonical volume is volume(); its weights stay what the class starts with unless given."""
    if cls is Fusion:
        o = Fusion(volume(), TDIST, marching_cubes_step_size=1, write_warpfield=False)
        o._K, o._Kinv = K, np.linalg.inv(K)
    else:
        o = FusionDM(TDIST, K, tsdf_res=R, marching_cubes_step_size=1, write_warpfield=False)
        o._tsdf = volume()
        o._IND = np.array([[0.5, 0, 0, 1.0], [0, 0.5, 0, -2.0], [0, 0, 0.5, 3.0], [0, 0, 0, 1.0]])
    if weights is not None:
        o._tsdfw = weights
    return o


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g, w.cpu().numpy() if isinstance(w, torch.Tensor) else w)


@BOTH
def test_marching_cubes_drops_the_blob(cls):
    o = make(cls)
    o.marching_cubes()
    v, f, n, _ = mesh.marching_cubes(o._T, None, 1)
    same((o._vertices, o._faces, o._normals), (v, f, n))
    o.min_component_faces = 20
    o.marching_cubes()
    v2, f2, n2, _ = mesh.filter_components(v, f, n, min_faces=20)
    same((o._vertices, o._faces, o._normals), (v2, f2, n2))
    assert 0 < len(f2) < len(f)
    live = np.roll(volume(), 1, axis=0)                         # a given volume: returned, nothing stored, never filtered
    same(o.marching_cubes(live, step_size=2), mesh.marching_cubes(torch.from_numpy(live).cuda(), None, 2))
    same((o._vertices, o._faces, o._normals), (v2, f2, n2))


@BOTH
def test_surface_samples(cls):
    band = 1.0 * SCALE
    o = make(cls, half_weights())
    o._faces = "stale"
    assert o.surface_samples(band=band) is None
    pos, nrm = extract_surface_samples(o._T, o._Wt, band)       # fused weights: both classes gate on them
    assert 0 < len(pos)
    same((o._vertices, o._normals), (pos, nrm))
    assert o._faces is None
    everywhere, _ = extract_surface_samples(o._T, torch.ones_like(o._T), band)
    assert len(pos) < len(everywhere)
    if cls is Fusion:                                           # never fused (all-zero weights): read with unit weights
        o = make(cls)
        o.surface_samples(band=band)
        assert float(o._Wt.max()) == 0.0
        same((o._vertices, o._normals), extract_surface_samples(o._T, torch.ones_like(o._T), band))
        assert o._faces is None and len(o._vertices) == len(everywhere)
    live = np.roll(volume(), 1, axis=0)
    got = o.surface_samples(live, band=band)
    lt = torch.from_numpy(live).cuda()
    pos, nrm = extract_surface_samples(lt, torch.ones_like(lt), band)
    assert got[1] is None and got[3] is None and len(got) == 4
    same((got[0], got[2]), (pos, nrm))


def color_volume(o):
    C = kernels.color_volume((R, R, R))
    rng = np.random.default_rng(7)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in LWS]
    kernels.integrate_color(C, o._T, o._Wt, [torch.from_numpy(d).cuda() for d in depth_maps()], images, K, np.linalg.inv(K),
                            LWS, SCALE, CENTER, TDIST, 1.5 * SCALE)
    assert bool((C[..., 3] > 0).any())
    return C


def write_abc(path, v, f, n, rgb=None):
    """Fusion's layout (reference core/fusion.py:577-587): index space, `f a b c`."""
    with open(path, "w") as fh:
        for i, p in enumerate(v):
            fh.write("v %f %f %f\n" % tuple(p) if rgb is None else "v %f %f %f %f %f %f\n" % (tuple(p) + tuple(rgb[i])))
        for p in n:
            fh.write("vn %f %f %f\n" % tuple(p))
        for t in f:
            fh.write("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1))


@BOTH
@pytest.mark.parametrize("branch", ["plain", "coloured", "simplified", "coloured simplified"])
def test_write_canonical_mesh(cls, branch, tmp_path):
    o = make(cls, np.ones((R, R, R), dtype=np.float32))
    o.marching_cubes(step_size=2)
    stored = [a.copy() for a in (o._vertices, o._faces, o._normals)]
    if "coloured" in branch:
        o._C = color_volume(o)
    if "simplified" in branch:
        o.simplify_cell = 2.0
    assert o.write_canonical_mesh(str(tmp_path), "got.obj") is None
    v, f, n, _ = mesh.marching_cubes(o._T, None if cls is Fusion else 0.0, 1)
    if "simplified" in branch:
        n_full = len(v)
        v, f, n, _ = mesh.simplify_with_normals(v, f, n, 2.0)
        assert 0 < len(v) < n_full
    rgb = valid = None
    if "coloured" in branch:
        rgb, valid = kernels.sample_colors(o._C, v.double())
        rgb, valid = rgb.cpu().numpy(), valid.cpu().numpy()
        assert valid.any()
    v, f, n = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()
    want = str(tmp_path / "want.obj")
    if cls is Fusion:
        write_abc(want, v, f, n, None if rgb is None else mesh.obj_colors(rgb, valid, len(v)))
    else:
        mesh.write_obj(want, v, f, n, ind=o._IND, **({} if rgb is None else dict(colors=rgb, valid=valid)))
    got = open(os.path.join(str(tmp_path), "got.obj"), "rb").read()
    assert got == open(want, "rb").read() and len(got) > 1000
    assert (b"//" in got) == (cls is FusionDM)
    same((o._vertices, o._faces, o._normals), stored)          # the stored mesh is not the file's


@BOTH
def test_volume_properties_round_trip(cls):
    vol, w = volume().astype(np.float64) + 1e-9, half_weights().astype(np.float64)
    if cls is Fusion:
        o = Fusion(np.zeros((4, 4, 4)), TDIST)
        assert o._tsdf_host is not None
        o._tsdf = vol                                           # before first use: the constructor's volume must not come back
        assert o._tsdf_host is None
    else:
        o = FusionDM(TDIST, K, tsdf_res=R)
        o._tsdf = vol
        assert not hasattr(o, "_tsdf_host")
    T, Wt = o.tsdf_device
    assert T is o._T and Wt is o._Wt and T.dtype == torch.float32 and T.is_cuda
    assert tuple(T.shape) == (R, R, R) and tuple(Wt.shape) == (R, R, R) and float(Wt.abs().max()) == 0.0
    assert o._tsdf.dtype == np.float64 and np.array_equal(o._tsdf, vol.astype(np.float32).astype(np.float64))
    o._tsdfw = w
    assert o._tsdfw.dtype == np.float64 and np.array_equal(o._tsdfw, w)
    o.marching_cubes(step_size=1)                               # ... and is the volume that gets used
    same((o._vertices, o._faces), mesh.marching_cubes(torch.from_numpy(vol).cuda().float(), None, 1)[:2])


@BOTH
def test_fuse_depths_numpy_and_tensor_volumes_agree(cls):
    o = make(cls)
    T, Wt = np.full((R, R, R), TDIST), np.zeros((R, R, R))
    Tc, Wc = torch.from_numpy(T).cuda().float(), torch.from_numpy(Wt).cuda().float()
    for d, lw in zip(depth_maps(), LWS):
        out = o.fuseDepths(d, lw, T, Wt, scale=SCALE, center=CENTER, wmax=1.5)
        assert out[0] is T and out[1] is Wt and T.dtype == np.float64
        outc = o.fuseDepths(torch.from_numpy(d).cuda(), lw, Tc, Wc, scale=SCALE, center=CENTER, wmax=1.5)
        assert outc[0] is Tc and outc[1] is Wc
    assert np.array_equal(T, Tc.cpu().numpy().astype(np.float64)) and np.array_equal(Wt, Wc.cpu().numpy().astype(np.float64))
    assert Wt.max() > 0 and (T < TDIST).any()
    arg = 'tsdfw' if cls is Fusion else 'tsdf_w'
    with pytest.raises(ValueError, match='^' + re.escape('tsdf and %s must both be numpy arrays or both CUDA tensors' % arg) + '$'):
        o.fuseDepths(depth_maps()[0], LWS[0], T, Wc)
    both_wrong = 'tsdf and tsdfw must both be numpy arrays or both CUDA tensors' if cls is Fusion else 'depth map must be 2-D'
    with pytest.raises(ValueError, match='^' + re.escape(both_wrong) + '$'):       # (each class keeps the order of its checks)
        o.fuseDepths(np.zeros(3), LWS[0], T, Wc)
    with pytest.raises(ValueError, match='^' + re.escape('tsdf and %s must be 3-D arrays of the same shape' % arg) + '$'):
        o.fuseDepths(depth_maps()[0], LWS[0], T, Wt[:-1])


@BOTH
def test_live_to_device_messages(cls):
    o = make(cls)
    np_text = 'Only accept 3D np array as tsdf'
    tensor_text = np_text if cls is Fusion else 'Only accept 3D array as tsdf'
    for bad, text in ((torch.zeros(4, 4), tensor_text), ([[[0.0]]], np_text), (np.zeros((4, 4)), np_text)):
        with pytest.raises(ValueError, match='^' + re.escape(text) + '$'):
            o._live_to_device(bad)
    t = o._live_to_device(np.full((2, 2, 2), 0.1))
    assert t.dtype == torch.float64 and t.is_cuda              # not float32-exact: travels as float64
    assert o._live_to_device(np.full((2, 2, 2), 0.5)).dtype == torch.float32
    assert o._live_to_device(torch.zeros(2, 2, 2, dtype=torch.int32)).dtype == torch.float32
