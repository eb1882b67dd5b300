"""GPU: the rasterizer (csrc/dfh_render.hip: render_small_kernel, render_large_kernel, render_resolve_kernel and the two readers
of the key buffer, samples_emit_kernel and render_vertex_ids_kernel) against the exact rational oracle (tests/raster_exact.py) on
the scenes of tests/raster_cases.py, whose projection is exact in fp64: boxes of exactly 64 and 65 pixels, boxes 255 / 256 / 257 /
300 pixels wide, a 37 x 29 box, a list longer than the raster grid, vertices and edges on pixel centres, coordinates on 0 / W - 1 /
znear, rejected faces, the vertex-id ties and the grey range's bounds.  tests/test_raster_exact.py ties the same oracle to the numpy
restatement without a device and shows, with a table of mutations, that the scenes bite.

Equal to the oracle: face map, depth bits, vertex ids, grey levels, the pixel list of the samples, and the listed (face, view)
pairs -- the count word and the list that dfh_render_raster leaves in its workspace (layout in include/dfusion_hip.h), which is what
shows that the large-triangle path ran.

Bounds.  A rendered normal component is within 2 float32 ulp of the oracle's (the bar of tests/test_gpu_render.py) or within 2^-40
absolute (the fp64 error budget of a unit vector's component that is nearly zero, where a float32 ulp means nothing).
Sample positions, from the operation count of the header's formula: in these scenes the edge values e_i and the area A are exact in
fp64, so with eps = 2^-53, lambda_i = e_i / A and a_i = lambda_i / z_i carry at most 2 eps, s = (a0 + a1) + a2 of non-negative
terms 2 + 2 = 4 eps, b_i = a_i / s 2 + 4 + 1 = 7 eps, each product b_i P_i 8 eps, the two additions 2 eps more:
|pos - exact| <= 10 eps sum_i b_i |P_i| <= 10 eps max|P| (b_i >= 0, sum 1); 12 eps max|P| with the oracle's final rounding and the
second-order terms.  A sample normal: every component of the interpolated m has the same bound delta = 12 eps max|N|, so
|dm| <= sqrt(3) delta, and a component of m / |m| moves by at most delta / |m| from its numerator and sqrt(3) delta / |m| from the
length: under 3 delta / |m|, plus 4 eps for the square root, the division and the oracle's two roundings.  The restatement's own
deviation from the oracle, printed by tests/test_raster_exact.py, is 2.67 eps max|P| and 0.06 of the normal bound at the most.
"""
import numpy as np
import pytest
import torch

import raster_cases as RC
import raster_exact as RX
from dynamicfusion_body_amd import _lib, mesh
from dynamicfusion_body_amd.device import current_stream_ptr

pytestmark = pytest.mark.gpu

RENDER_BLOCK = 256                                       # kRenderBlock of csrc/dfh_render.hip


def listed(ws, n_views, H, W):
    """The listed pairs dfh_render_raster left in workspace `ws` (layout in include/dfusion_hip.h: the keys, then 16-byte aligned
    one uint32 count, then 16-byte aligned the list): (count, the entries sorted)."""
    words = ws.buf.view(torch.int32)
    at = ((n_views * H * W * 8 + 15) // 16 * 16) // 4
    n = int(words[at].item())
    return n, sorted(words[at + 4:at + 4 + n].cpu().numpy().astype(np.int64).tolist())


def expected_list(s, o):
    return sorted(v * len(s.faces) + f for v, f in o.large)


def render(s, workspace=None):
    """mesh.render of the scene's first 16 views into `workspace`: (depth, normal, face as numpy, the workspace)."""
    nv = min(len(s.views), RC.RENDER_MAX_VIEWS)
    ws = workspace or mesh.render_workspace(nv, s.H, s.W, len(s.faces))
    d, n, f = mesh.render(s.verts, s.faces, s.normals, s.Ks()[:nv], s.lws()[:nv], s.H, s.W, znear=s.znear, workspace=ws, **s.geom)
    return d.cpu().numpy(), n.cpu().numpy(), f.cpu().numpy(), ws


def same_maps(name, depth, face, o):
    assert np.array_equal(face, o.face), "%s: face map differs in %d pixels" % (name, (face != o.face).sum())
    assert np.array_equal(depth.view(np.uint32), o.depth.view(np.uint32)), "%s: depth bits differ in %d pixels" % (
        name, (depth.view(np.uint32) != o.depth.view(np.uint32)).sum())


@pytest.mark.parametrize("name", RC.NAMES)
def test_maps_and_listed_pairs_equal_the_oracle(name):
    s, o = RC.scene(name), RC.oracle(name)
    nv = o.depth.shape[0]
    depth, normal, face, ws = render(s)
    n, entries = listed(ws, nv, s.H, s.W)
    print("%s: %d covered pixels, %d listed pairs of %d" % (name, (face >= 0).sum(), n, nv * len(s.faces)))
    assert n == len(o.large) and entries == expected_list(s, o)
    same_maps(name, depth, face, o)
    ex = RX.normal_excess(normal, o.normal)
    print("%s: normals at %.3g of the allowance" % (name, ex))
    assert ex <= 1.0 and not normal[o.face < 0].any()


@pytest.mark.parametrize("name", RC.NAMES)
def test_samples_equal_the_oracle(name):
    s, o = RC.scene(name), RC.oracle(name)
    nv = o.depth.shape[0]
    pos, nrm, pix = mesh.render_samples(s.verts, s.faces, s.cpos, s.cnrm, s.Ks()[:nv], s.lws()[:nv], s.H, s.W, znear=s.znear, **s.geom)
    pos, nrm, pix = pos.cpu().numpy(), nrm.cpu().numpy(), pix.cpu().numpy()
    assert np.array_equal(pix, o.pixel)
    bp, bn = RX.sample_bounds(s, o)
    dp = np.abs(pos - o.pos).max() if len(pix) else 0.0
    dn = (np.abs(nrm - o.nrm) / bn).max() if len(pix) else 0.0
    print("%s: %d samples, |pos - oracle| max %.3g (bound %.3g), normals at %.3g of their bound" % (name, len(pix), dp, bp, dn))
    assert dp <= bp and dn <= 1.0


@pytest.mark.parametrize("name", RC.NAMES)
def test_vertex_ids_and_grey_levels_equal_the_oracle(name):
    """Every view of the scene (views_17: two batches of the wrapper)."""
    s, o = RC.scene(name), RC.oracle(name)
    vid, grey = mesh.render_vertex_ids(s.verts, s.faces, s.Ks(), s.lws(), s.H, s.W, *s.img, znear=s.znear, **s.geom)
    assert vid.shape[0] == len(s.views)
    assert np.array_equal(vid.cpu().numpy(), o.vid), "vid differs in %d pixels" % (vid.cpu().numpy() != o.vid).sum()
    assert np.array_equal(grey.cpu().numpy(), o.grey), "grey differs in %d pixels" % (grey.cpu().numpy() != o.grey).sum()


def test_all_large_list_is_longer_than_the_grid():
    """780 listed pairs on min(ceil(780 / 256), 4 CUs) = 4 workgroups: the stride loop of render_large_kernel goes round about
    195 times, and a workgroup of render_small_kernel spans two views (260 faces per view)."""
    s, o = RC.scene("all_large"), RC.oracle("all_large")
    pairs = len(s.views) * len(s.faces)
    grid = min(-(-pairs // RENDER_BLOCK), 4 * torch.cuda.get_device_properties(0).multi_processor_count)
    assert len(o.large) == pairs == 780 and grid == 4 and len(s.faces) % RENDER_BLOCK != 0
    _, _, _, ws = render(s)
    assert listed(ws, len(s.views), s.H, s.W) == (pairs, list(range(pairs)))


def test_sixteen_views_in_one_call_equal_single_calls():
    s, o = RC.scene("views_16"), RC.oracle("views_16")
    depth, normal, face, _ = render(s)
    same_maps("views_16", depth, face, o)
    for vi, vw in enumerate(s.views):
        d, n, f = mesh.render(s.verts, s.faces, s.normals, vw.K(), vw.lw(), s.H, s.W, znear=s.znear, **s.geom)
        assert np.array_equal(d[0].cpu().numpy().view(np.uint32), depth[vi].view(np.uint32)) and np.array_equal(f[0].cpu().numpy(), face[vi])
        assert np.array_equal(n[0].cpu().numpy().view(np.uint32), normal[vi].view(np.uint32))


def test_sheet_is_watertight():
    """Non-dyadic input: a jittered sheet with a row of slivers 1e-13 high, a skewed K, three turned views.  Coverage is decided
    exactly on the projected doubles; a pixel is exempt only within the rounding bound of an edge expression."""
    verts, faces, K, lws, geom = RC.sheet()
    face = mesh.render(verts, faces, None, K, lws, RC.SHEET_H, RC.SHEET_W, **geom)[2].cpu().numpy()
    covered, exempt, bad = RC.watertight_report(face)
    print("sheet: %d contained pixels, %d exempt" % (covered, exempt))
    assert covered > 500 and exempt <= 0.005 * covered
    assert bad == [], bad[:5]


@pytest.mark.parametrize("first, second", [("large_few", "switch_boxes"), ("switch_boxes", "large_few")])
def test_workspace_reuse(first, second):
    """Two scenes of one image size through one caller-supplied workspace that starts out as garbage: the second's maps and
    listed pairs are those of a fresh workspace (a stale count, a stale list, stale keys)."""
    a, b = RC.scene(first), RC.scene(second)
    assert (len(a.views), a.H, a.W) == (len(b.views), b.H, b.W)
    ws = mesh.render_workspace(len(a.views), a.H, a.W, max(len(a.faces), len(b.faces)))
    ws.buf.fill_(0x5A5A5A5A5A5A5A5A)
    depth, _, face, _ = render(a, ws)
    same_maps(first, depth, face, RC.oracle(first))
    assert listed(ws, len(a.views), a.H, a.W) == (len(RC.oracle(first).large), expected_list(a, RC.oracle(first)))
    depth, normal, face, _ = render(b, ws)
    same_maps(second, depth, face, RC.oracle(second))
    assert listed(ws, len(b.views), b.H, b.W) == (len(RC.oracle(second).large), expected_list(b, RC.oracle(second)))
    assert len(RC.oracle(first).large) != len(RC.oracle(second).large)
    fresh = render(b)
    assert np.array_equal(fresh[0].view(np.uint32), depth.view(np.uint32)) and np.array_equal(fresh[2], face)
    assert np.array_equal(fresh[1].view(np.uint32), normal.view(np.uint32))


GUARD = 1024                                             # guard elements either side of every output


def _guarded(n, dtype, pattern):
    buf = torch.full((n + 2 * GUARD,), pattern, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


@pytest.mark.parametrize("name", ["all_large", "image_1x1"])
def test_outputs_stay_inside_their_arrays(name):
    """The raw C calls with every output between guard words: the maps equal the oracle's and the guards are intact."""
    s, o = RC.scene(name), RC.oracle(name)
    lib = _lib.load()
    nv = len(s.views)
    npix = nv * s.H * s.W
    dev, V, F, msh, views, ws = mesh._render_args(s.verts, s.faces, s.Ks(), s.lws(), s.H, s.W, s.geom["scale"], s.geom["center"],
                                                  s.geom["half"], s.znear, None)
    Nn = torch.from_numpy(np.array(s.normals)).to(dev)
    outs = {"depth": _guarded(npix, torch.float32, 7.5), "face": _guarded(npix, torch.int32, -7),
            "normal": _guarded(3 * npix, torch.float32, 7.5), "vid": _guarded(npix, torch.int32, -7),
            "image": _guarded(npix, torch.uint8, 0xA5)}
    before = {k: b.clone() for k, (b, _) in outs.items()}
    st = current_stream_ptr()
    _lib.check(lib.dfh_render_raster(*msh, *views, st), "dfh_render_raster")
    _lib.check(lib.dfh_render_resolve(V.data_ptr(), Nn.data_ptr(), *msh[1:], *views, outs["depth"][1].data_ptr(), outs["face"][1].data_ptr(),
                                      outs["normal"][1].data_ptr(), st), "dfh_render_resolve")
    _lib.check(lib.dfh_render_vertex_ids(*msh, *views, float(s.img[0]), float(s.img[1]), outs["vid"][1].data_ptr(),
                                         outs["image"][1].data_ptr(), st), "dfh_render_vertex_ids")
    torch.cuda.synchronize()
    for k, (buf, _) in outs.items():
        assert torch.equal(buf[:GUARD], before[k][:GUARD]) and torch.equal(buf[-GUARD:], before[k][-GUARD:]), "%s: guard overwritten" % k
    shape = (nv, s.H, s.W)
    same_maps(name, outs["depth"][1].cpu().numpy().reshape(shape), outs["face"][1].cpu().numpy().reshape(shape), o)
    assert np.array_equal(outs["vid"][1].cpu().numpy().reshape(shape), o.vid)
    assert np.array_equal(outs["image"][1].cpu().numpy().reshape(shape), o.grey)
    assert RX.normal_excess(outs["normal"][1].cpu().numpy().reshape(shape + (3,)), o.normal) <= 1.0
