"""The call surface of Fusion / FusionDM after their shared code moved into canonical.CanonicalModel: every name and signature
the two classes had before is still there, the non-rigid methods FusionDM used to be lent are inherited, and
device.depths_to_device states the list dtype rule.  No device is needed."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dynamicfusion_body_amd
from dynamicfusion_body_amd import Fusion, FusionDM, canonical, device, fusion, fusion_dm

# name -> str(inspect.signature) (None: not callable) for every name of dir(cls) without a leading "__", as the two classes stood
# before the shared base (generated from that commit by the loop of _surface() below)
SURFACE = {
    'Fusion': {
        'InitializeCanonicalSpace': '(self, tsdf=None, depths=None, lws=None, K=None, tsdf_size=256, scale=1.0, center=array([0., 0., 0.]), colors=None, color_band=1.5)',
        '_blend_warp_batch': '(self, V, Nn, nbr)',
        '_canonical_mesh_device': '(self)',
        '_dq_blend_kdtree': '(self, pos)',
        '_dqb_warp': '(dq, p)',
        '_ensure_volumes': '(self)',
        '_gather_nodes': '(self, locations, dqs)',
        '_live_to_device': '(self, curr_tsdf)',
        '_locations': '(self, pos, k)',
        '_tsdf': None,
        '_tsdfw': None,
        '_vertex_state': '(self)',
        '_write_back': '(self, sv)',
        '_write_mesh_file': '(fpath, verts, faces, normals, rgb=None)',
        'average_edge_dist_in_face': '(self, f)',
        'computeSparsity': '(self, n, m)',
        'computef': '(self, x, tdw, trw, rw)',
        'computef_lw': '(self, x, tdw, trw)',
        'construct_graph': '(self)',
        'depth_prep': None,
        'descriptor_fn': None,
        'dq_blend': '(self, pos, dqs=None, locations=None, dmax=None)',
        'fuseDepths': '(self, dm, lw, tsdf, tsdfw, wmax=100.0, scale=1.0, center=array([0., 0., 0.]))',
        'graph_sampler': None,
        'ingest': None,
        'initialize_canonical': '(self)',
        'live_frame_mesh': '(self, nodes=None)',
        'marching_cubes': '(self, tsdf=None, step_size=0)',
        'node_arrays': '(self)',
        'render_canonical': '(self, lws, H, W, K=None, scale=1.0, center=array([0., 0., 0.]), **kw)',
        'render_live_frame': '(self, lws, H, W, K=None, scale=1.0, center=array([0., 0., 0.]), nodes=None)',
        'setupCorrespondences': "(self, curr_tsdf, method='cnn', prune_result=True, tolerance=0.2, live_vertices=None, descriptors=None)",
        'solve': "(self, correspondences=None, method='cnn', precompute_lw=True, tukey_data_weight=0.2, huber_regularization_weight=0.001, regularization_weight=1, iterations=10, pcg_iters=30, huber_delta=1.0)",
        'surface_samples': '(self, tsdf=None, band=1.0)',
        'tsdf_device': None,
        'updateTSDF': '(self, curr_tsdf=None, wmax=100.0)',
        'updateTSDF_depths': "(self, depths, lws, wmax=100.0, weight='node_distance', scale=1.0, center=array([0., 0., 0.]), colors=None, color_band=1.5)",
        'update_graph': '(self, refresh_surface=True)',
        'volume_from_mesh': '(self, verts, faces, band=None, orientation=1)',
        'warp': '(self, pos, dqs=None, locations=None, normal=None, dmax=None, m_lw=None)',
        'write_canonical_mesh': '(self, path, filename)',
        'write_live_frame_mesh': '(self, path, filename, warpfield_path)',
        'write_warp_field': '(self, path, filename)',
    },
    'FusionDM': {
        '_auto_alignment': '(self, depths, lws)',
        '_canonical_mesh_device': '(self)',
        '_corr_state': '(self)',
        '_depth_to_device': '(self, dm)',
        '_dq_blend_kdtree': '(self, pos)',
        '_dqb_warp': '(dq, p)',
        '_ensure_volumes': '(self)',
        '_gather_nodes': '(self, locations, dqs)',
        '_live_to_device': '(self, curr_tsdf)',
        '_locations': '(self, pos, k)',
        '_new_volume_pair': '(self, res=None)',
        '_tsdf': None,
        '_tsdfw': None,
        '_vertex_state': '(self)',
        'average_edge_dist_in_face': '(self, f)',
        'computeSparsity': '(self, n, m)',
        'compute_live_tsdf': "(self, depths, lws, UseAutoAlignment=False, useICP=False, outputMesh=False, as_numpy=True, mesh_path='.', colors=None, color_band=1.5)",
        'computef': '(self, x, tdw, trw, rw)',
        'computef_lw': '(self, x)',
        'construct_graph': '(self)',
        'depth_prep': None,
        'dq_blend': '(self, pos, dqs=None, locations=None, dmax=None)',
        'fuseDepths': "(self, dm, lw, tsdf, tsdf_w, scale=1.0, center=array([0., 0., 0.]), wmax=100.0, mode='cpu')",
        'fuseDepths_ocl': '(self, dm, lw, tsdf, tsdf_w, wmax=100.0)',
        'graph_sampler': None,
        'ingest': None,
        'live_frame_mesh': '(self, nodes=None)',
        'marching_cubes': '(self, tsdf=None, step_size=1)',
        'node_arrays': '(self)',
        'render_live_frame': '(self, lws, H, W, K=None, scale=1.0, center=array([0., 0., 0.]), nodes=None)',
        'render_model': '(self, lws, H, W, K=None, scale=1.0, center=array([0., 0., 0.]), **kw)',
        'setupCorrespondences': '(self, curr_tsdf, prune_result=True, tolerance=1.0, live_vertices=None)',
        'solve': '(self, curr_tsdf=None, iterations=10)',
        'surface_samples': '(self, tsdf=None, band=1.0)',
        'track_frame': '(self, depths, lws_prev, tracker, scale=1.0, center=array([0., 0., 0.]), **kw)',
        'tsdf_device': None,
        'updateTSDF': '(self, curr_tsdf, wmax=100.0)',
        'update_graph': '(self, refresh_surface=True)',
        'verbose_gpu': '(self)',
        'warp': '(self, pos, dqs=None, locations=None, normal=None, dmax=None, m_lw=None)',
        'write_canonical_mesh': '(self, path, filename)',
        'write_live_frame_mesh': '(self, path, filename, warpfield_path)',
        'write_warp_field': '(self, path, filename)',
    },
}

# the constructors (dir() lists them with a leading "__", so they are pinned here)
CTORS = {
    'Fusion': '(self, tsdf, trunc_distance, subsample_rate=5.0, knn=4, marching_cubes_step_size=3, verbose=False, use_cnn=False, '
              'write_warpfield=True, volume_dtype=<class \'numpy.float32\'>)',
    'FusionDM': '(self, trunc_distance, K, tsdf_res=256, subsample_rate=5.0, knn=4, marching_cubes_step_size=3, verbose=False, '
                'write_warpfield=True, volume_dtype=<class \'numpy.float32\'>)',
}

# what the shared base added; all private.  Anything else that appears on a class fails test_surface_is_what_it_was.
NEW_SHARED = {'_init_model', '_prepare_depths', '_check_volume_pair', '_fuse_depth_into', '_raycast_canonical', '_marching_cubes',
              '_write_mesh', '_mc_level', '_live_tensor_error', '_weight_arg', '_unit_weight_samples'}
NEW = {'Fusion': NEW_SHARED | {'_dqb_workspace_for'}, 'FusionDM': NEW_SHARED}

LENT = ("node_arrays", "_gather_nodes", "_locations", "dq_blend", "_dqb_warp", "warp", "_vertex_state", "computef",
        "computeSparsity", "construct_graph", "_dq_blend_kdtree", "update_graph", "live_frame_mesh", "render_live_frame")

CLASSES = {'Fusion': Fusion, 'FusionDM': FusionDM}


def _surface(cls):
    out = {}
    for n in dir(cls):
        if not n.startswith("__"):
            a = getattr(cls, n)
            out[n] = str(inspect.signature(a)) if callable(a) else None
    return out


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_surface_is_what_it_was(name):
    now = _surface(CLASSES[name])
    was = SURFACE[name]
    assert not set(was) - set(now), "names lost"
    assert {n: now[n] for n in was} == was
    assert set(now) - set(was) == NEW[name]
    assert all(n.startswith("_") for n in NEW[name])
    assert str(inspect.signature(CLASSES[name].__init__)) == CTORS[name]
    for n in ("_tsdf", "_tsdfw", "tsdf_device"):
        assert isinstance(inspect.getattr_static(CLASSES[name], n), property)
    assert inspect.getattr_static(CLASSES[name], "_tsdf").fset is not None
    assert inspect.getattr_static(CLASSES[name], "_tsdfw").fset is not None
    assert inspect.getattr_static(CLASSES[name], "tsdf_device").fset is None


def test_package_exports():
    assert dynamicfusion_body_amd.__all__ == ["Fusion", "FusionDM", "FusionDM_GPU", "scene"]
    assert dynamicfusion_body_amd.FusionDM_GPU is FusionDM
    assert fusion._is_tensor is canonical._is_tensor and fusion_dm._is_tensor is canonical._is_tensor
    assert Fusion.graph_sampler == "host" and FusionDM.graph_sampler == "host"
    assert (Fusion.marching_cubes.__defaults__, FusionDM.marching_cubes.__defaults__) == ((None, 0), (None, 1))


def test_lent_methods_are_inherited():
    """The fourteen methods fusion.py used to setattr on FusionDM at import: one object on both classes, defined on neither."""
    assert not hasattr(fusion, "_lend_nonrigid_methods")
    assert issubclass(Fusion, canonical.CanonicalModel) and issubclass(FusionDM, canonical.CanonicalModel)
    assert type(Fusion) is type and type(FusionDM) is type and type(canonical.CanonicalModel) is type
    for n in LENT + ("graph_sampler",):
        assert getattr(FusionDM, n) is getattr(Fusion, n), n
        assert n not in FusionDM.__dict__ and n not in Fusion.__dict__, n
        assert n in canonical.CanonicalModel.__dict__, n


def test_fusion_dm_module_is_complete_alone():
    """`import dynamicfusion_body_amd.fusion_dm` in a fresh interpreter, where fusion.py has not been imported: the class has
    the names it has after importing the whole package."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(dynamicfusion_body_amd.__file__)))
    # (the package's __init__ imports fusion.py too: the module is loaded under a bare package object that runs no __init__)
    code = ("import importlib, sys, types\n"
            "pkg = types.ModuleType('dynamicfusion_body_amd'); pkg.__path__ = [%r]\n"
            "sys.modules['dynamicfusion_body_amd'] = pkg\n"
            "m = importlib.import_module('dynamicfusion_body_amd.fusion_dm')\n"
            "assert 'dynamicfusion_body_amd.fusion' not in sys.modules\n"
            "print('\\n'.join(dir(m.FusionDM)))\n" % os.path.join(root, "dynamicfusion_body_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == dir(FusionDM)


def test_constructors_need_no_device():
    f = Fusion(np.zeros((4, 4, 4)), 0.1)
    g = FusionDM(0.1, np.eye(3), tsdf_res=4)
    for o in (f, g):
        assert o._T is None and o._Wt is None and o._C is None
        assert o._vol_dtype == torch.float32 and o._nodes == [] and o._vertices is None
    assert f._tsdf_host is not None and not hasattr(g, "_tsdf_host")
    assert f._lw[5] == np.float32(0.1) and g._lw[5] == 0
    with pytest.raises(ValueError, match='^Only 3D numpy array is accepted as tsdf$'):
        Fusion(np.zeros((4, 4)), 0.1)
    with pytest.raises(ValueError, match='^intrinsic matrix K must be 3x3$'):
        FusionDM(0.1, np.eye(4))


def test_new_module_keeps_the_product_rules():
    """What tests/test_abi_symbols.py asks of fusion.py and fusion_dm.py holds for the module their code moved to."""
    import re
    txt = open(canonical.__file__).read()
    assert "os.environ" not in txt and "import oracle" not in txt and "from oracle" not in txt
    assert not re.search(r"import\s+c?KDTree|scipy\.spatial", txt)


INEXACT = np.float64(0.1)                                      # not a float32 value


@pytest.mark.parametrize("maps, want", [
    ([np.ones((2, 3), np.float32), np.zeros((2, 3), np.float32)], torch.float32),
    ([np.full((2, 3), 0.5), np.full((2, 3), -1.25)], torch.float32),                         # float64, float32-exact
    ([np.full((2, 3), 0.5), np.full((2, 3), INEXACT), np.ones((2, 3), np.float32)], torch.float64),
])
def test_depths_to_device_dtype_rule(monkeypatch, maps, want):
    """float32 unless some float64 map is not float32-exact; then EVERY map of the call goes as float64."""
    sent = []
    monkeypatch.setattr(device, "to_device", lambda a, dtype=None, device=None: sent.append((a, dtype)) or len(sent) - 1)
    assert device.depths_dtype(maps) == want
    assert device.depths_to_device(maps) == list(range(len(maps)))
    assert [d for _, d in sent] == [want] * len(maps)
    assert all(a is m for (a, _), m in zip(sent, maps))
    assert device.depths_dtype(maps[:1]) == torch.float32 and device.depths_dtype([maps[0], INEXACT]) == torch.float64
