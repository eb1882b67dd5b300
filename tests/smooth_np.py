"""The numpy restatement of K25 (mesh smoothing by Taubin's lambda|mu filter over a fixed Laplacian, and area-weighted vertex
normals), operation by operation as include/dfusion_hip.h defines it: fp64, one rounding per operation (every line below is one
elementwise numpy operation per arithmetic operation: no cross, einsum, matmul or linalg, which may fuse or reorder), sums from
0.0 in the stated order.  The loops are explicit and ordered: round j adds the j-th entry of every vertex's list that has one, so
every vertex's accumulator takes its entries in ascending order, one after the other.  The device must equal it bit for bit."""
import numpy as np


def taubin_mu(lam, pass_band):
    return 1.0 / (float(pass_band) - 1.0 / float(lam))


class Laplacian:
    """The prepared mesh: lists (begin, end, a, b per sorted entry), boundary flags, weights from the positions given here."""

    def __init__(self, verts, faces, weights="uniform", boundary="fixed"):
        assert weights in ("uniform", "cotangent") and boundary in ("fixed", "free")
        verts = np.asarray(verts)
        self.dtype = verts.dtype
        self.p = p = verts.astype(np.float64).reshape(-1, 3)
        faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
        self.V, self.F = V, F = len(p), len(faces)
        if not np.isfinite(p).all():
            raise ValueError("a vertex coordinate is not finite")
        if F and (faces.min() < 0 or faces.max() >= V):
            raise ValueError("a face holds a vertex index outside [0, V)")
        self.weights, self.fixed = weights, boundary == "fixed"
        ent = faces.reshape(-1)                              # entry e = 3 f + corner names vertex ent[e]
        order = np.argsort(ent, kind="stable")
        self.v = v = ent[order]
        f, c = order // 3, order % 3
        self.a = faces[f, (c + 1) % 3] if F else np.zeros(0, dtype=np.int64)
        self.b = faces[f, (c + 2) % 3] if F else np.zeros(0, dtype=np.int64)
        self.begin = np.searchsorted(v, np.arange(V), side="left")
        self.end = np.searchsorted(v, np.arange(V), side="right")
        self.deg = self.end - self.begin
        self.rounds = []                                     # round j: the vertices whose list has a j-th entry, and that entry
        for j in range(int(self.deg.max()) if V else 0):
            idx = np.nonzero(self.deg > j)[0]
            self.rounds.append((idx, self.begin[idx] + j))
        self.boundary = np.zeros(V, dtype=bool)
        for u in range(V):
            lst = np.stack([self.a[self.begin[u]:self.end[u]], self.b[self.begin[u]:self.end[u]]], axis=1).reshape(-1)
            names, counts = np.unique(lst[lst != u], return_counts=True)
            self.boundary[u] = bool((counts != 2).any())
        self.wa = self.wb = None
        if weights == "cotangent":
            self.wa, self.wb = self._cotangents()
            self.W = np.zeros(V)
            for idx, i in self.rounds:
                self.W[idx] = self.W[idx] + self.wa[i]
                self.W[idx] = self.W[idx] + self.wb[i]
        else:
            self.W = (2 * self.deg).astype(np.float64)

    def _cotangents(self):
        pv, pa, pb = self.p[self.v], self.p[self.a], self.p[self.b]
        e1, e2 = pa - pv, pb - pv
        n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        A2 = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)

        def weight(d, g):
            with np.errstate(all="ignore"):
                q = ((d[:, 0] * g[:, 0] + d[:, 1] * g[:, 1]) + d[:, 2] * g[:, 2]) / A2
            return np.where((A2 > 0) & (q > 0), q, 0.0)
        return weight(pv - pb, pa - pb), weight(pv - pa, pb - pa)

    def step(self, x, factor):
        """One pass over x (V, K) float64."""
        acc = np.zeros_like(x)
        for idx, i in self.rounds:
            da, db = x[self.a[i]] - x[idx], x[self.b[i]] - x[idx]
            if self.wa is not None:
                da, db = self.wa[i][:, None] * da, self.wb[i][:, None] * db
            acc[idx] = acc[idx] + da
            acc[idx] = acc[idx] + db
        move = self.W > 0
        if self.fixed:
            move = move & ~self.boundary
        with np.errstate(all="ignore"):
            new = x + np.float64(factor) * (acc / self.W[:, None])
        return np.where(move[:, None], new, x)

    def smooth(self, x=None, iters=10, lam=0.5, mu=None, pass_band=0.1):
        mu = taubin_mu(lam, pass_band) if mu is None else float(mu)
        x = self.p.astype(self.dtype) if x is None else np.asarray(x)
        y = x.astype(np.float64).reshape(self.V, int(np.prod(x.shape[1:])))
        for _ in range(iters):
            y = self.step(y, lam)
            if mu != 0.0:
                y = self.step(y, mu)
        return y.astype(x.dtype).reshape(x.shape)

    def vertex_normals(self, verts=None, sign=1.0):
        verts = self.p.astype(self.dtype) if verts is None else np.asarray(verts)
        p = verts.astype(np.float64)
        s = np.zeros((self.V, 3))
        for idx, i in self.rounds:
            e1, e2 = p[self.a[i]] - p[idx], p[self.b[i]] - p[idx]
            s[idx, 0] = s[idx, 0] + (e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1])
            s[idx, 1] = s[idx, 1] + (e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2])
            s[idx, 2] = s[idx, 2] + (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])
        m = np.float64(sign) * s
        length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        with np.errstate(all="ignore"):
            n = m / length[:, None]
        return np.where((length > 0)[:, None], n, 0.0).astype(verts.dtype)


def smooth(verts, faces, iters=10, weights="uniform", boundary="fixed", **kw):
    return Laplacian(verts, faces, weights, boundary).smooth(None, iters, **kw)


def vertex_normals(verts, faces, sign=1.0):
    return Laplacian(verts, faces).vertex_normals(None, sign)


# ---- what the golden records (tools/make_smooth_golden.py writes it, tests/test_smooth_np.py reproduces it) --------------------
def radial(verts, centre):
    d = np.asarray(verts, dtype=np.float64) - np.asarray(centre, dtype=np.float64)
    return np.sqrt((d * d).sum(axis=1))


def recovery_measures(noisy, faces, taubin, laplace, centre, radius):
    r0, rt, rl = radial(noisy, centre), radial(taubin, centre), radial(laplace, centre)
    rms = lambda r: float(np.sqrt(((r - r.mean()) ** 2).mean()))
    return {"rms_radial_deviation_before": rms(r0), "rms_radial_deviation_after_taubin": rms(rt),
            "mean_radius_before": float(r0.mean()), "mean_radius_shift_taubin": float(rt.mean() - r0.mean()),
            "mean_radius_shift_laplace": float(rl.mean() - r0.mean()), "n_verts": int(len(noisy)), "n_faces": int(len(faces))}


def golden_record(noisy, faces, centre, radius, smoother=smooth):
    """Ten Taubin iterations (uniform, lam 0.5, pass band 0.1) and twenty plain Laplacian passes (mu = 0) on the noisy icosphere."""
    taubin = smoother(noisy, faces, 10, lam=0.5, pass_band=0.1)
    laplace = smoother(noisy, faces, 20, lam=0.5, mu=0.0)
    return recovery_measures(noisy, faces, np.asarray(taubin), np.asarray(laplace), centre, radius)
