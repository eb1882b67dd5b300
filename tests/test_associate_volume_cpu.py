"""CPU: what dfh_gn_associate_volume does with arguments it cannot use, and what the Python layers of the volume data term
refuse before they load or launch anything.  Validation comes before any HIP call, so no GPU is needed: device pointers are
dummy non-null integers that nothing dereferences (as in tests/test_abi_badargs.py)."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

from dynamicfusion_body_amd import _lib, build
from dynamicfusion_body_amd.pipeline import SlabFrame
from dynamicfusion_body_amd.solve import WarpSolver

OK, BADARG = 0, -1
PTR = 0x1000                                    # a "device pointer"
NAME = b"dfh_gn_associate_volume"
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def on_own_thread(test):
    """dfh_last_error() is kept per thread: the refused calls are made on a thread of their own."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        with ThreadPoolExecutor(1) as ex:
            return ex.submit(test, *args, **kwargs).result()
    return run


def problem(**over):
    p = _lib.Problem()
    for f in ("sample_pos", "sample_nrm", "nbr", "weights", "corr", "valid", "node_dq"):
        setattr(p, f, PTR)
    p.n_samples, p.knn, p.n_nodes = 5, 4, 8
    p.lw_dq = (ctypes.c_double * 8)(1.0)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def term(data=PTR, dtype=_lib.F32, res=(4, 4, 4), value_to_vox=1.0, band=4.0, max_dist=0.0, min_grad=0.5):
    return _lib.VolumeTerm(_lib.Live(data, dtype, _lib.iarr(res)), value_to_vox, band, max_dist, min_grad)


BAD = {
    "null problem": lambda: (None, term()),
    "null term": lambda: (problem(), None),
    "null sample_pos": lambda: (problem(sample_pos=0), term()),
    "null nbr": lambda: (problem(nbr=0), term()),
    "null weights": lambda: (problem(weights=0), term()),
    "null node_dq": lambda: (problem(node_dq=0), term()),
    "null corr": lambda: (problem(corr=0), term()),
    "null valid": lambda: (problem(valid=0), term()),
    "null live.data": lambda: (problem(), term(data=0)),
    "knn 0": lambda: (problem(knn=0), term()),
    "knn 9": lambda: (problem(knn=9), term()),
    "n_nodes 0": lambda: (problem(n_nodes=0), term()),
    "n_samples -1": lambda: (problem(n_samples=-1), term()),
    "dtype 2": lambda: (problem(), term(dtype=2)),
    "dtype -1": lambda: (problem(), term(dtype=-1)),
    "res[0] 1": lambda: (problem(), term(res=(1, 4, 4))),
    "res[1] 1": lambda: (problem(), term(res=(4, 1, 4))),
    "res[2] 0": lambda: (problem(), term(res=(4, 4, 0))),
    "value_to_vox 0": lambda: (problem(), term(value_to_vox=0.0)),
    "value_to_vox nan": lambda: (problem(), term(value_to_vox=NAN)),
    "value_to_vox inf": lambda: (problem(), term(value_to_vox=INF)),
    "band 0": lambda: (problem(), term(band=0.0)),
    "band -1": lambda: (problem(), term(band=-1.0)),
    "band nan": lambda: (problem(), term(band=NAN)),
    "min_grad -1": lambda: (problem(), term(min_grad=-1.0)),
    "min_grad nan": lambda: (problem(), term(min_grad=NAN)),
}


@pytest.mark.parametrize("case", sorted(BAD))
@on_own_thread
def test_bad_arguments_are_refused(lib, case):
    p, t = BAD[case]()
    rc = lib.dfh_gn_associate_volume(p, t, None)
    assert rc == BADARG, (case, rc)
    assert NAME in lib.dfh_last_error(), (case, lib.dfh_last_error())


@on_own_thread
def test_no_samples_is_ok_without_a_launch(lib):
    assert lib.dfh_gn_associate_volume(problem(n_samples=0), term(), None) == OK
    # (a rank whose slab holds no surface has empty sample tensors, whose data pointers are null)
    assert lib.dfh_gn_associate_volume(problem(n_samples=0, sample_pos=0, nbr=0, weights=0, corr=0, valid=0), term(dtype=_lib.F64), None) == OK
    # ... but the term is still checked
    assert lib.dfh_gn_associate_volume(problem(n_samples=0), term(band=0.0), None) == BADARG


def test_python_layers_refuse_before_loading_anything(monkeypatch):
    """A bad data_term, a live volume that is not on the device, and one that is not contiguous: ValueError before the
    library is loaded or a GPU is asked for (the objects are not even constructed)."""
    def no_load(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    frame = object.__new__(SlabFrame)
    with pytest.raises(ValueError, match="data_term"):
        frame.step(None, None, data_term="sdf")
    sv = object.__new__(WarpSolver)
    ident = [1.0, 0, 0, 0, 0, 0, 0, 0]
    cpu = torch.zeros((4, 4, 4), dtype=torch.float32)
    for call in (lambda v: sv.associate_volume(v, ident, 4.0), lambda v: sv.iterate_volume(v, ident, 5.0, 4.0)):
        with pytest.raises(ValueError, match="live"):
            call(cpu)                                         # not a CUDA tensor
        with pytest.raises(ValueError, match="live"):
            call(cpu.permute(2, 1, 0)[:, :, ::2])             # nor contiguous
        with pytest.raises(ValueError, match="live"):
            call(cpu.numpy())                                 # nor a tensor at all
