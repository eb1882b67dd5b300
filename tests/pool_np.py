"""numpy restatement of K15 (semantics: include/dfusion_hip.h, dfh_render_vertex_ids and dfh_pool_features), and the integer
formulas behind tests/golden/g10_pool.npz (no random generator's stream: the inputs are functions of the pixel index).

vertex_ids stands on tests/render_np.py: its keys (as the depth and face maps), its set-up and its edge values.
pool_features is the loop of core/sdf.py:138-149, one float32 addition per pixel and channel in ascending pixel order."""
import numpy as np

import render_np as R


# ---- dfh_render_vertex_ids ---------------------------------------------------------------------------------------------------------
def winner(a0, a1, a2):
    """The reference's fragment-shader rule on the perspective-correct coordinates."""
    return np.where((a0 > a1) & (a0 > a2), 0, np.where(a1 > a2, 1, 2))


def image_from_depth(d, znear_img, zfar_img):
    """float32 depths d -> uint8 grey levels; 0 outside [znear_img, zfar_img] (compared in fp64)."""
    d = np.asarray(d, dtype=np.float32)
    zf, zn = np.float32(zfar_img), np.float32(znear_img)
    with np.errstate(all="ignore"):
        g = ((zf - d) / (zf - zn)) * np.float32(255)
        inside = (d.astype(np.float64) >= znear_img) & (d.astype(np.float64) <= zfar_img)
        grey = np.clip(np.where(inside, g, np.float32(0)).astype(np.int64), 0, 255)
    return np.where(inside, grey, 0).astype(np.uint8)


def vertex_ids(verts, faces, K, lws, H, W, znear_img, zfar_img, scale=1.0, center=0.0, half=0.0, znear=1e-3):
    """Same call shape and results as mesh.render_vertex_ids, as numpy arrays: (vid (V,H,W) int32, image (V,H,W) uint8).
    K one 3x3 or one per view."""
    verts = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    lws = np.asarray(lws, dtype=np.float64)
    if lws.ndim == 2:
        lws = lws[None]
    nv = len(lws)
    Ks = np.asarray(K, dtype=np.float64)
    if Ks.ndim == 2:
        Ks = np.broadcast_to(Ks, (nv, 3, 3))
    vid = np.full((nv, H, W), -1, dtype=np.int32)
    image = np.zeros((nv, H, W), dtype=np.uint8)
    for vi in range(nv):
        depth, _, face = R.render(verts, faces, None, Ks[vi], lws[vi], H, W, scale, center, half, znear)
        depth, face = depth[0], face[0]
        d = -depth                                                    # the float32 in the key's high bits
        hit = face >= 0
        image[vi] = np.where(hit, image_from_depth(d, znear_img, zfar_img), 0)
        inside = hit & (d.astype(np.float64) >= znear_img) & (d.astype(np.float64) <= zfar_img)
        with np.errstate(all="ignore"):
            U, Vv, Z = R.project(verts, Ks[vi], lws[vi], scale, center, half)
        for f in np.unique(face[inside]):
            idx = faces[f]
            u, v, z = U[idx], Vv[idx], Z[idx]
            A = R.setup(u, v, z, H, W, znear)[0]
            ys, xs = np.nonzero(inside & (face == f))
            _, l0, l1, l2 = R.bary(u, v, A, xs.astype(np.float64), ys.astype(np.float64))
            w = winner(l0 / z[0], l1 / z[1], l2 / z[2])
            vid[vi, ys, xs] = idx[w]
    return vid, image


# ---- dfh_pool_features ---------------------------------------------------------------------------------------------------------------
def pool_features(vid, feats, n_verts, descending=False):
    """(feat (n_verts, D) float32, cnt (n_verts,) int32).  The k-th pixel of every vertex is added in round k (one float32
    addition per vertex, channel and round: the loop of the definition, vectorised over the vertices).
    descending=True sums every vertex's pixels in DESCENDING order instead: what a wrong order looks like."""
    vid = np.asarray(vid).reshape(-1).astype(np.int64)
    feats = np.asarray(feats, dtype=np.float32)
    feats = feats.reshape(len(vid), feats.shape[-1])
    D = feats.shape[1]
    p = np.flatnonzero((vid >= 0) & (vid < n_verts))
    if descending:
        p = p[::-1]
    p = p[np.argsort(vid[p], kind="stable")]
    v = vid[p]
    cnt = np.bincount(v, minlength=n_verts).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    rank = np.arange(len(p)) - start[v]
    by_round = np.argsort(rank, kind="stable")
    p, v = p[by_round], v[by_round]
    ends = np.cumsum(np.bincount(rank, minlength=1))
    acc = np.zeros((n_verts, D), dtype=np.float32)
    with np.errstate(all="ignore"):
        lo = 0
        for hi in ends:
            acc[v[lo:hi]] = acc[v[lo:hi]] + feats[p[lo:hi]]          # (a vertex appears once per round)
            lo = hi
        seen = cnt > 0
        acc[seen] = acc[seen] / cnt[seen].astype(np.float32)[:, None]
    return acc, cnt


def pool_features_loop(vid, feats, n_verts):
    """The definition word for word (slow): for checking pool_features on small inputs."""
    vid = np.asarray(vid).reshape(-1)
    feats = np.asarray(feats, dtype=np.float32)
    feats = feats.reshape(len(vid), feats.shape[-1])
    acc = np.zeros((n_verts, feats.shape[1]), dtype=np.float32)
    cnt = np.zeros(n_verts, dtype=np.int32)
    with np.errstate(all="ignore"):
        for p in range(len(vid)):
            if 0 <= vid[p] < n_verts:
                cnt[vid[p]] += 1
                acc[vid[p]] += feats[p]
        for v in range(n_verts):
            if cnt[v] > 0:
                acc[v] = acc[v] / np.float32(cnt[v])
    return acc, cnt


# ---- the golden's inputs (tests/golden/make_golden_pool.py, tests/golden/g10_pool.npz) ----------------------------------------------
G_VIEWS, G_H, G_W, G_DIM = 24, 512, 512, 16
G_VERTS, G_FACES = 300, 200
G_ZNEAR, G_ZFAR = 1.0, 3.5
G_WINDOW = 128                                                        # the covered pixels of a view lie in one square window


def _hash(view, salt):
    """A 32-bit integer per pixel of the view: a multiplicative hash of the pixel index, the view and `salt`."""
    q = np.arange(G_H * G_W, dtype=np.uint64).reshape(G_H, G_W)
    h = (q * np.uint64(2654435761) + np.uint64(view * 40503 + salt * 69069 + 12345)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    return h.astype(np.int64)


def _window(view):
    y0, x0 = (view * 37) % (G_H - G_WINDOW), (view * 91) % (G_W - G_WINDOW)
    m = np.zeros((G_H, G_W), dtype=bool)
    m[y0:y0 + G_WINDOW, x0:x0 + G_WINDOW] = True
    return m


def golden_ids(view):
    """(H, W) int32: the vertex of every pixel of `view`, -1 where there is none (a quarter of the window is covered)."""
    h = _hash(view, 1)
    return np.where(_window(view) & (h % 4 == 0), (h // 4) % G_VERTS, -1).astype(np.int32)


def golden_features(view):
    """(H, W, 16) float32: integers of up to 1000 times powers of two from 2^-6 to 2^5 (all exact), so that partial sums round
    and the order of a vertex's additions decides the low bits of its mean."""
    out = np.empty((G_H, G_W, G_DIM), dtype=np.float32)
    for c in range(G_DIM):
        h = _hash(view, 2 + c)
        out[:, :, c] = ((h % 2001) - 1000).astype(np.float64) * 2.0 ** ((h // 2001) % 12 - 6)
    return out


def golden_z(view):
    """(H, W) float32 GL depth buffer: 1 (the far plane) except on a sixteenth of the window, where it is the buffer value
    a + b / d of a camera depth d strictly between znear and zfar."""
    b = G_ZFAR * G_ZNEAR / (G_ZNEAR - G_ZFAR)
    a = -b / G_ZNEAR
    h = _hash(view, 99)
    d = G_ZNEAR + (G_ZFAR - G_ZNEAR) * ((h // 16) % 4096 + 0.5) / 4096.0
    return np.where(_window(view) & (h % 16 == 0), a + b / d, 1.0).astype(np.float32)


def golden_depth_from_z(z):
    """fp64 camera depth of a GL depth-buffer value (the inverse the reference applies, core/sdf.py:135)."""
    b = G_ZFAR * G_ZNEAR / (G_ZNEAR - G_ZFAR)
    a = -b / G_ZNEAR
    return b / (np.asarray(z, dtype=np.float64) - a)


def golden_mesh():
    """(vertices (300,3) float64, faces (200,3) int32): points of an integer lattice scaled to a body's proportions."""
    i = np.arange(G_VERTS, dtype=np.int64)
    verts = np.stack([(i * 7919) % 211 - 105, (i * 104729) % 601 - 300, (i * 1299709) % 157 - 78], axis=1).astype(np.float64)
    verts = verts * np.array([0.004, 0.003, 0.002]) + np.array([0.3, -0.2, 0.1])
    j = np.arange(G_FACES, dtype=np.int64)
    faces = np.stack([(j * 3) % G_VERTS, (j * 5 + 1) % G_VERTS, (j * 11 + 2) % G_VERTS], axis=1).astype(np.int32)
    return verts, faces
