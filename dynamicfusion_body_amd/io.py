"""File formats on either side of the hot path, host-side like in the
reference: the `.dist` signed-distance volumes (reference core/sdf.py:24-69), the `proj*.txt`
camera matrices (core/util.py:330-335) and the warp-field pickle (core/fusion.py:571-573)."""
import os
import pickle

import numpy as np


def load_sdf(file_path, read_closest_points=False, verbose=False):
    """Reference core/sdf.py:24-69.  Layout: int32 -res_x, int32 -res_y, int32 res_z (the first two
    are stored negated), 3 float64 b_min, 3 float64 b_max, (1+res)^3 float32 distances stored
    z-major (reshaped (1+res_z, 1+res_y, 1+res_x) and swapped to x-major), optionally 3 float32
    closest-point coordinates per grid vertex.  Returns (b_min, b_max, volume, closest_points)."""
    with open(file_path, 'rb') as fp:
        head = np.fromfile(fp, dtype=np.int32, count=3)
        if head.size != 3:
            raise ValueError('%s: truncated .dist header' % file_path)
        res_x, res_y, res_z = -int(head[0]), -int(head[1]), int(head[2])
        if verbose:
            print("resolution: %d %d %d" % (res_x, res_y, res_z))
        b_min = np.fromfile(fp, dtype=np.float64, count=3)
        b_max = np.fromfile(fp, dtype=np.float64, count=3)
        grid_num = (1 + res_x) * (1 + res_y) * (1 + res_z)
        volume = np.fromfile(fp, dtype=np.float32, count=grid_num)
        if b_min.size != 3 or b_max.size != 3 or volume.size != grid_num:
            raise ValueError('%s: truncated .dist body' % file_path)
        volume = np.swapaxes(volume.reshape(((1 + res_z), (1 + res_y), (1 + res_x))), 0, 2)
        closest_points = None
        if read_closest_points:
            cp = np.fromfile(fp, dtype=np.float32, count=grid_num * 3)
            if cp.size != grid_num * 3:
                raise ValueError('%s: truncated closest-point block' % file_path)
            closest_points = np.swapaxes(cp.reshape(((1 + res_z), (1 + res_y), (1 + res_x), 3)), 0, 2)
    return b_min, b_max, volume, closest_points


def write_sdf(file_path, b_min, b_max, volume, closest_points=None):
    """Inverse of load_sdf (the reference only reads this format)."""
    vol = np.asarray(volume, dtype=np.float32)
    rx, ry, rz = (s - 1 for s in vol.shape)
    with open(file_path, 'wb') as fp:
        np.array([-rx, -ry, rz], dtype=np.int32).tofile(fp)
        np.asarray(b_min, dtype=np.float64).tofile(fp)
        np.asarray(b_max, dtype=np.float64).tofile(fp)
        np.ascontiguousarray(np.swapaxes(vol, 0, 2)).tofile(fp)
        if closest_points is not None:
            np.ascontiguousarray(np.swapaxes(np.asarray(closest_points, dtype=np.float32), 0, 2)).tofile(fp)


def read_proj_matrix(fpath):
    """Reference core/util.py:330-335: whitespace-free, single-space separated rows of floats
    (every line must end with a newline, which the reference strips blindly)."""
    arr = []
    with open(fpath, 'r') as f:
        for line in f:
            arr.append(line[:-1].split(' '))
    return np.array(arr, dtype='float')


def write_warp_field(nodes, path, filename, itercounter):
    """Reference core/fusion.py:571-573: pickle of the `_nodes` list of 4-tuples
    (vertex index, position, dual quaternion, weight) to <path>/<filename>__<iter>.p."""
    fname = os.path.join(path, filename + '__' + str(itercounter) + '.p')
    with open(fname, 'wb') as f:
        pickle.dump(nodes, f)
    return fname


def read_warp_field(fname):
    """Files written by write_warp_field of THIS package (never unpickle untrusted files)."""
    with open(fname, 'rb') as f:
        return pickle.load(f)


# ---- binary Netpbm: what a raw RGB-D capture can be stored in without an image library (ingest.RGBDIngest's inputs) ----
def _netpbm_header(buf, magic, path):
    """(width, height, maxval, offset of the raster) of a binary Netpbm file: whitespace-separated decimal fields, '#' comments to
    the end of the line, ONE whitespace byte after maxval."""
    if buf[:2] != magic:
        raise ValueError('%s: not a binary %s file' % (path, magic.decode()))
    pos, fields = 2, []
    while len(fields) < 3:
        while pos < len(buf) and (buf[pos:pos + 1].isspace() or buf[pos:pos + 1] == b'#'):
            if buf[pos:pos + 1] == b'#':
                while pos < len(buf) and buf[pos:pos + 1] not in (b'\n', b'\r'):
                    pos += 1
            else:
                pos += 1
        end = pos
        while end < len(buf) and buf[end:end + 1].isdigit():
            end += 1
        if end == pos:
            raise ValueError('%s: bad Netpbm header' % path)
        fields.append(int(buf[pos:end]))
        pos = end
    if not buf[pos:pos + 1].isspace():
        raise ValueError('%s: bad Netpbm header' % path)
    return fields[0], fields[1], fields[2], pos + 1


def read_pgm16(path):
    """A binary PGM (P5) with maxval 256..65535 -> (H, W) uint16 (the samples are big-endian in the file)."""
    with open(path, 'rb') as f:
        buf = f.read()
    w, h, maxval, off = _netpbm_header(buf, b'P5', path)
    if not 255 < maxval <= 65535:
        raise ValueError('%s: maxval %d is not a 16-bit PGM (256..65535)' % (path, maxval))
    if len(buf) - off < 2 * w * h:
        raise ValueError('%s: truncated raster' % path)
    return np.frombuffer(buf, dtype='>u2', count=w * h, offset=off).reshape(h, w).astype(np.uint16)


def write_pgm16(path, image):
    """(H, W) uint16 -> binary PGM (P5), maxval 65535, big-endian samples."""
    a = np.asarray(image)
    if a.ndim != 2 or a.dtype != np.uint16:
        raise ValueError('write_pgm16 takes an (H, W) uint16 array')
    with open(path, 'wb') as f:
        f.write(b'P5\n%d %d\n65535\n' % (a.shape[1], a.shape[0]))
        f.write(a.astype('>u2').tobytes())


def read_ppm(path):
    """A binary PPM (P6) with maxval 255 -> (H, W, 3) uint8."""
    with open(path, 'rb') as f:
        buf = f.read()
    w, h, maxval, off = _netpbm_header(buf, b'P6', path)
    if maxval != 255:
        raise ValueError('%s: maxval %d is not an 8-bit PPM' % (path, maxval))
    if len(buf) - off < 3 * w * h:
        raise ValueError('%s: truncated raster' % path)
    return np.frombuffer(buf, dtype=np.uint8, count=3 * w * h, offset=off).reshape(h, w, 3).copy()


def write_ppm(path, image):
    """(H, W, 3) uint8 -> binary PPM (P6), maxval 255."""
    a = np.asarray(image)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError('write_ppm takes an (H, W, 3) uint8 array')
    with open(path, 'wb') as f:
        f.write(b'P6\n%d %d\n255\n' % (a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a).tobytes())


def mesh_to_dist(path, verts, faces, res, b_min=None, b_max=None, margin=0.1, orientation=+1):
    """Write the reference-format `.dist` file of a mesh: the exact signed distance (mesh.MeshDistance, band = inf) and the
    closest surface point at the (1 + res)^3 grid vertices of the box [b_min, b_max] (default: the mesh's box grown by `margin`
    on every side).  res: one integer or three.  Returns (b_min, b_max, volume, closest_points) as load_sdf would."""
    from . import mesh
    res = np.broadcast_to(np.asarray(res, dtype=np.int64), (3,))
    if res.min() < 1:
        raise ValueError("res must be at least 1")
    md = mesh.MeshDistance(verts, faces, orientation=orientation)
    v = np.asarray(verts.detach().cpu().numpy() if hasattr(verts, "detach") else verts, dtype=np.float64)
    b_min = v.min(axis=0) - margin if b_min is None else np.asarray(b_min, dtype=np.float64).reshape(3)
    b_max = v.max(axis=0) + margin if b_max is None else np.asarray(b_max, dtype=np.float64).reshape(3)
    if not (np.isfinite(b_min).all() and np.isfinite(b_max).all() and (b_max > b_min).all()):
        raise ValueError("the box must be finite with b_max > b_min")
    vol, cp = md.grid(b_min, (b_max - b_min) / res, tuple(int(r) + 1 for r in res), float("inf"), dtype=np.float32, want_closest=True)
    vol, cp = vol.cpu().numpy(), cp.cpu().numpy()
    write_sdf(path, b_min, b_max, vol, cp)
    return b_min, b_max, vol, cp
