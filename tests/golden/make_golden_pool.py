#!/usr/bin/env python3
"""Builds tests/golden/g10_pool.npz from the reference's own compute_correspondence (core/sdf.py:95-150).  Runs in the build
container only (python -B tests/golden/make_golden_pool.py from the repository root); the .npz travels.

The reference's renderer and network are replaced by stubs: `GLRenderer.draw` returns supplied (rgb, z) images and records what
it was handed, `sess.run` returns supplied features and records the image it was fed.  Everything else -- the mesh
normalisation, the 24 cameras, the depth-to-image expression, the pooling loop and the final division -- is the reference's code.
The supplied images are the integer formulas of tests/pool_np.py.

Content:
  feat    (300, 16) float32   what compute_correspondence returned
  mvp     (24, 4, 4) float32  the matrices handed to draw (transposed back: clip = mvp @ [x, y, z, 1])
  vbuf    (600, 3) float64    the regularised vertex buffer handed to draw (vertices[faces])
  images  (24, 512, 512) u8   the images fed to the session for the stub's z buffers
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_import  # noqa: E402
import pool_np as PN  # noqa: E402


def main():
    if not ref_import.available():
        print("reference tree not present: nothing written")
        return
    ref_import.load()
    import core.sdf as sdf

    seen = {"mvp": [], "vbuf": None, "images": []}

    class StubRenderer:
        def __init__(self, *args, **kwargs):
            self.view = 0

        def draw(self, vertices, colors, mvp):
            seen["mvp"].append(np.array(mvp, dtype=np.float32).T.copy())
            seen["vbuf"] = np.array(vertices)
            ids = PN.golden_ids(self.view).astype(np.int64) + 1       # the reference's colours are 1-based, 0 = background
            rgb = np.stack([ids // 65536 % 256, ids // 256 % 256, ids % 256], axis=-1).astype(np.uint8)
            z = PN.golden_z(self.view)
            self.view += 1
            return rgb, z

    class StubSession:
        def __init__(self):
            self.view = 0

        def run(self, feature, feed_dict):
            (image,) = feed_dict.values()
            seen["images"].append(np.array(image).reshape(PN.G_H, PN.G_W).copy())
            out = PN.golden_features(self.view)
            self.view += 1
            return out

    sdf.GLRenderer = StubRenderer
    verts, faces = PN.golden_mesh()
    feat = sdf.compute_correspondence("input", "feature", StubSession(), verts.copy(), faces.copy(), znear=PN.G_ZNEAR, zfar=PN.G_ZFAR,
                                      width=PN.G_W, height=PN.G_H)
    assert feat.dtype == np.float32 and feat.shape == (PN.G_VERTS, PN.G_DIM)
    assert len(seen["mvp"]) == PN.G_VIEWS and len(seen["images"]) == PN.G_VIEWS
    images = np.stack(seen["images"])
    assert images.dtype == np.uint8

    # the fixture must be able to see a wrong order: the restatement reproduces it, the descending sum does not
    vid = np.stack([PN.golden_ids(v) for v in range(PN.G_VIEWS)])
    feats = np.stack([PN.golden_features(v) for v in range(PN.G_VIEWS)])
    up, cnt = PN.pool_features(vid, feats, PN.G_VERTS)
    down, _ = PN.pool_features(vid, feats, PN.G_VERTS, descending=True)
    assert np.array_equal(up.view(np.uint32), feat.view(np.uint32)), "the restatement does not reproduce the reference"
    differ = int((up.view(np.uint32) != down.view(np.uint32)).sum())
    assert differ > 0, "the features do not make the order visible"
    out = os.path.join(HERE, "g10_pool.npz")
    np.savez_compressed(out, feat=feat, mvp=np.stack(seen["mvp"]), vbuf=seen["vbuf"].astype(np.float64), images=images)
    print("wrote", out, os.path.getsize(out), "bytes; pixels per vertex %d..%d; %d of %d words differ in descending order"
          % (cnt.min(), cnt.max(), differ, feat.size))


if __name__ == "__main__":
    main()
