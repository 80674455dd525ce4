"""Float64 statement (plain numpy) of the surface mesh of a scalar volume -- TEST INFRASTRUCTURE ONLY, the arbiter of
csrc/gnr_mesh.hip -- naive surface nets over the iso-surface vol = iso (include/gnr.h, gnr_surface_mesh_fwd, has the same words).
Vectorised over the cells; the 12 edges of a cell are visited one after the other in the statement's order and a cell that an edge does
not cross adds +0.0 to its sums, which changes no bit of them (a sum that started at +0.0 is never -0.0).  Every operation below is one
IEEE float64 operation, so the device's results are compared with np.array_equal."""
import numpy as np


def _edges():
    """The 12 edges of a cell in the statement's order: (a, offset of p0)."""
    for a in (0, 1, 2):
        b, c = (a + 1) % 3, (a + 2) % 3
        for dc in (0, 1):
            for db in (0, 1):
                o = [0, 0, 0]
                o[b], o[c] = db, dc
                yield a, tuple(o)


def surface_mesh(vol, iso=0.0, scale=1.0, origin=(0.0, 0.0, 0.0), gradient=None):
    """vol [R,R,R] -> dict: vertices [N,3] float64, faces [F,3] int32, (gradient [N,3] float32), cells [N] the vertices' cell indices."""
    vol = np.ascontiguousarray(vol, np.float32)
    R = vol.shape[0]
    assert vol.shape == (R, R, R) and R >= 2
    C = R - 1
    iso32 = np.float32(iso)
    isod, scale = np.float64(iso32), np.float64(scale)
    inside = vol < iso32                                                     # float32 comparison; a value equal to iso is outside
    v64 = vol.astype(np.float64)
    sl = lambda o: tuple(slice(k, k + C) for k in o)
    n_in = np.zeros((C, C, C), np.int64)
    for k in range(8):
        n_in += inside[sl((k >> 2, (k >> 1) & 1, k & 1))]
    active = (n_in > 0) & (n_in < 8)
    grid = np.indices((C, C, C))
    ssum, n = np.zeros((3, C, C, C)), np.zeros((C, C, C))
    if gradient is not None:
        g64 = np.ascontiguousarray(gradient, np.float32).astype(np.float64)
        assert g64.shape == (R, R, R, 3)
        gsum = np.zeros((C, C, C, 3))
    for a, o0 in _edges():
        o1 = tuple(o0[k] + (k == a) for k in range(3))
        cross = inside[sl(o0)] != inside[sl(o1)]
        v0, v1 = v64[sl(o0)], v64[sl(o1)]
        with np.errstate(divide='ignore', invalid='ignore'):
            t = np.where(cross, (isod - v0) / (v1 - v0), 0.0)
        for k in range(3):
            pk = (grid[k] + o0[k]).astype(np.float64)                        # p0, exact
            if k == a:
                pk = pk + t
            ssum[k] += np.where(cross, pk, 0.0)
        n += cross
        if gradient is not None:
            g0, g1 = g64[sl(o0)], g64[sl(o1)]
            gsum += np.where(cross[..., None], g0 + t[..., None] * (g1 - g0), 0.0)
    cells = np.flatnonzero(active.ravel())                                   # ascending x (R-1)^2 + y (R-1) + z
    nn = n.ravel()[cells]
    assert (nn > 0).all()
    mean = np.stack([ssum[k].ravel()[cells] / nn for k in range(3)], 1)
    out = {'cells': cells, 'vertices': np.asarray(origin, np.float64)[None, :] + mean * scale}
    if gradient is not None:
        out['gradient'] = (gsum.reshape(-1, 3)[cells] / nn[:, None]).astype(np.float32)
    row = np.full(C ** 3, -1, np.int64)
    row[cells] = np.arange(len(cells))
    keys, tris = [], []
    P = np.indices((R, R, R))
    for a in (0, 1, 2):
        b, c = (a + 1) % 3, (a + 2) % 3
        nxt = np.zeros_like(inside)
        src = [slice(None)] * 3
        dst = [slice(None)] * 3
        src[a], dst[a] = slice(1, R), slice(0, R - 1)
        nxt[tuple(dst)] = inside[tuple(src)]
        sel = (P[a] <= R - 2) & (P[b] >= 1) & (P[b] <= R - 2) & (P[c] >= 1) & (P[c] <= R - 2) & (inside != nxt)
        p = np.argwhere(sel)                                                 # [K,3]
        if not len(p):
            continue
        eb, ec = np.eye(3, dtype=np.int64)[b], np.eye(3, dtype=np.int64)[c]
        lin = lambda q: row[(q[:, 0] * C + q[:, 1]) * C + q[:, 2]]
        q0, q1, q2, q3 = lin(p - eb - ec), lin(p - ec), lin(p), lin(p - eb)
        rising = inside[p[:, 0], p[:, 1], p[:, 2]]                           # p inside: vol rises along +a
        t1 = np.where(rising[:, None], np.stack([q0, q1, q2], 1), np.stack([q0, q2, q1], 1))
        t2 = np.where(rising[:, None], np.stack([q0, q2, q3], 1), np.stack([q0, q3, q2], 1))
        keys.append(((p[:, 0] * R + p[:, 1]) * R + p[:, 2]) * 3 + a)
        tris.append(np.stack([t1, t2], 1))                                   # [K,2,3]
    if keys:
        keys, tris = np.concatenate(keys), np.concatenate(tris)
        faces = tris[np.argsort(keys, kind='stable')].reshape(-1, 3)
    else:
        faces = np.zeros((0, 3), np.int64)
    assert (faces >= 0).all()
    out['faces'] = faces.astype(np.int32)
    return out


# ---- inputs of the tests: signed distances on the voxel grid, float32 ----
def sphere(R, centre, r):
    g = np.indices((R, R, R)).astype(np.float64)
    return (np.sqrt(sum((g[k] - centre[k]) ** 2 for k in range(3))) - r).astype(np.float32)


def torus(R, centre, major, minor):
    g = np.indices((R, R, R)).astype(np.float64)
    x, y, z = (g[k] - centre[k] for k in range(3))
    return (np.sqrt((np.sqrt(x * x + y * y) - major) ** 2 + z * z) - minor).astype(np.float32)


def plane(R, normal=(0.31, 0.52, 0.8), offset=6.3):
    g = np.indices((R, R, R)).astype(np.float64)
    nrm = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    return (sum(g[k] * nrm[k] for k in range(3)) - offset).astype(np.float32)


# ---- properties of a mesh ----
def edge_counts(faces):
    """-> (undirected edge -> triangles, directed edge -> triangles) as dicts of counts."""
    und, dire = {}, {}
    for tri in np.asarray(faces).tolist():
        for i in range(3):
            u, v = tri[i], tri[(i + 1) % 3]
            dire[(u, v)] = dire.get((u, v), 0) + 1
            k = (min(u, v), max(u, v))
            und[k] = und.get(k, 0) + 1
    return und, dire


def euler_characteristic(n_vertices, faces):
    return n_vertices - len(edge_counts(faces)[0]) + len(faces)


def signed_volume(vertices, faces):
    a, b, c = (vertices[faces[:, k]] for k in range(3))
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)
