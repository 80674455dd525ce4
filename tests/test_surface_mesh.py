"""Surface mesh of the SDF volume on the device (csrc/gnr_mesh.hip, grasp_post.MeshExtractor, plan_real(mesh=True)): naive surface
nets over vol = iso.  tests/mesh_reference.py is the statement in numpy float64; the device's counts, vertices, faces and gradient
rows are compared with it by np.array_equal on the bits.  Without a GPU: the invariants of the statement itself (closed, oriented,
Euler characteristic, distance from the analytic surface), the refusals made before the device is touched, and write_ply's faces."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib
from graspnerf_amd.grasp_post import MeshExtractor, mesh_bounds, mesh_from_extraction, write_ply
import mesh_reference as ref

SPHERES = [(6, (2.3, 2.6, 2.45), 1.7), (8, (3.3, 3.6, 3.45), 2.4), (10, (4.3, 4.6, 4.45), 3.2)]
TORUS = (16, (7.3, 7.6, 7.45), 4.5, 2.0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---- the statement's invariants (no GPU) ---------------------------------------------------------------------------------------
def _closed_and_oriented(m):
    und, dire = ref.edge_counts(m['faces'])
    assert set(und.values()) == {2}, 'an undirected edge is not in exactly two triangles'
    assert set(dire.values()) == {1}, 'a directed edge appears twice: the orientation is inconsistent'
    f = m['faces']
    assert not ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any()
    assert f.min() >= 0 and f.max() < len(m['vertices'])


@pytest.mark.parametrize('R,centre,r', SPHERES)
def test_sphere_is_closed_oriented_and_near_the_sphere(R, centre, r):
    m = ref.surface_mesh(ref.sphere(R, centre, r))
    _closed_and_oriented(m)
    assert ref.euler_characteristic(len(m['vertices']), m['faces']) == 2
    assert ref.signed_volume(m['vertices'], m['faces']) > 0                     # normals out of the object
    dist = np.abs(np.linalg.norm(m['vertices'] - np.asarray(centre), axis=1) - r).max()
    print(f'R = {R}: {len(m["vertices"])} vertices, {len(m["faces"])} triangles, farthest vertex {dist:.3f} voxel from the sphere')
    assert dist <= 0.25


def test_torus_two_spheres_and_a_plane_that_leaves_the_grid():
    R, centre, major, minor = TORUS
    m = ref.surface_mesh(ref.torus(R, centre, major, minor))
    _closed_and_oriented(m)
    assert ref.euler_characteristic(len(m['vertices']), m['faces']) == 0
    two = np.minimum(ref.sphere(12, (3.3, 3.6, 3.45), 2.2), ref.sphere(12, (8.3, 8.1, 8.2), 2.1))
    m = ref.surface_mesh(two)
    _closed_and_oriented(m)
    assert ref.euler_characteristic(len(m['vertices']), m['faces']) == 4
    R = 16
    m = ref.surface_mesh(ref.plane(R))
    und, dire = ref.edge_counts(m['faces'])
    assert set(dire.values()) == {1} and set(und.values()) == {1, 2}
    C = R - 1
    cell = np.stack([m['cells'] // (C * C), (m['cells'] // C) % C, m['cells'] % C], 1)
    border = ((cell == 0) | (cell == C - 1)).any(1)
    for (u, v), k in und.items():
        if k == 1:
            assert border[u] and border[v], 'a boundary edge inside the grid'


def test_smallest_grid_and_a_value_equal_to_iso():
    vol = np.ones((2, 2, 2), np.float32)
    vol[0, 0, 0] = -1.0
    m = ref.surface_mesh(vol)
    assert len(m['faces']) == 0 and m['faces'].dtype == np.int32 and m['vertices'].shape == (1, 3)
    assert np.abs(m['vertices'] - 1.0 / 6.0).max() <= 1e-16
    vol[vol > 0] = 0.0                                                          # equal to iso: outside; t = 1 on every crossing edge
    m = ref.surface_mesh(vol)
    assert m['vertices'].shape == (1, 3) and np.abs(m['vertices'] - 1.0 / 3.0).max() <= 1e-16
    assert len(ref.surface_mesh(np.zeros((3, 3, 3), np.float32))['vertices']) == 0      # all equal to iso: all outside
    g = np.indices((9, 9, 9)).astype(np.float64)
    vol = (np.sqrt(((g - 4.0) ** 2).sum(0)) - 3.0).astype(np.float32)             # integer centre and radius: exact zeros on the axes
    assert (vol == 0).sum() >= 6
    m = ref.surface_mesh(vol, iso=0.0, scale=0.5, origin=(1.0, -2.0, 3.0))
    assert np.isfinite(m['vertices']).all() and len(m['vertices']) > 0
    _closed_and_oriented(m)


# ---- the C ABI's refusals, before the device (no GPU) --------------------------------------------------------------------------
def test_refusals_before_the_device():
    """Fake pointers: every call is one that validation refuses, each with its code and a text that names the limit."""
    L = _lib.lib()
    one, big = C.c_void_p(16), C.c_size_t(1 << 60)
    good = _lib.GnrMeshParams(iso=0.0, scale=1.0)

    def call(B=1, R=8, p=good, vol=one, grad=None, count=one, vertices=one, faces=one, gradient=None, max_v=8, max_f=8, ws=one, nbytes=big):
        return L.gnr_surface_mesh_fwd(vol, grad, B, R, C.byref(p) if p is not None else None, count, vertices, faces, gradient, max_v, max_f,
                                      ws, nbytes, None)

    text = lambda: L.gnr_last_error().decode()
    for name in ('vol', 'count', 'vertices', 'faces', 'ws', 'p'):
        assert call(**{name: None}) == _lib.GNR_ERR_ARG, name
        assert text() == 'gnr_surface_mesh_fwd: null pointer', name
    for kw in (dict(grad=one), dict(gradient=one)):
        assert call(**kw) == _lib.GNR_ERR_ARG and 'both given or both NULL' in text(), kw
    for B in (0, -1, 65536):
        assert call(B=B) == _lib.GNR_ERR_SHAPE and '1..65535' in text(), B
    for R in (1, 0, 257):
        assert call(R=R) == _lib.GNR_ERR_SHAPE and '2..256' in text(), R
    assert call(max_v=0) == _lib.GNR_ERR_SHAPE and 'max_v must be >= 1' in text()
    assert call(max_f=0) == _lib.GNR_ERR_SHAPE and 'max_f must be >= 1' in text()
    for bad in (dict(iso=float('nan')), dict(iso=float('inf')), dict(scale=float('-inf')), dict(scale=float('nan'))):
        assert call(p=_lib.GnrMeshParams(**{**dict(iso=0.0, scale=1.0), **bad})) == _lib.GNR_ERR_ARG and 'finite' in text(), bad
    for k in range(3):
        p = _lib.GnrMeshParams(iso=0.0, scale=1.0)
        p.origin[k] = float('nan')
        assert call(p=p) == _lib.GNR_ERR_ARG and 'finite' in text(), k
    for B, R in ((1, 8), (3, 40), (2, 256)):
        need = L.gnr_surface_mesh_workspace_bytes(B, R)
        nc = (R - 1) ** 3
        assert need >= 4 * B * (nc + -(-nc // 1024) + -(-R ** 3 // 1024))         # the map and the two tables of chunk counts
        assert call(B=B, R=R, nbytes=C.c_size_t(need - 1)) == _lib.GNR_ERR_WORKSPACE, (B, R)
        assert 'gnr_surface_mesh_workspace_bytes' in text()
    assert L.gnr_surface_mesh_workspace_bytes(1, 1) == 0 and L.gnr_surface_mesh_workspace_bytes(0, 8) == 0


def test_extractor_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(_lib.GnrError, match='no CPU fallback'):
        MeshExtractor()


def test_mesh_bounds_and_mesh_from_extraction_on_host_tensors():
    assert mesh_bounds(2) == (1, 1) and mesh_bounds(40) == (39 ** 3, 6 * 39 * 38 ** 2)
    m = ref.surface_mesh(ref.sphere(*SPHERES[0]))
    nv, nf = len(m['vertices']), len(m['faces'])
    g = np.random.default_rng(0).standard_normal((nv + 2, 3)).astype(np.float32)
    res = {'count': torch.tensor([[nv, nf]], dtype=torch.int32), 'vertices': torch.zeros(1, nv + 2, 3, dtype=torch.float64),
           'faces': torch.zeros(1, nf + 1, 3, dtype=torch.int32), 'gradient': torch.from_numpy(g)[None]}
    res['vertices'][0, :nv] = torch.from_numpy(m['vertices'])
    res['faces'][0, :nf] = torch.from_numpy(m['faces'])
    out = mesh_from_extraction(res, 0)
    assert same(out['vertices'], m['vertices']) and out['faces'].dtype == np.int64 and np.array_equal(out['faces'], m['faces'])
    assert same(out['gradient'], g[:nv]) and np.abs(np.linalg.norm(out['normals'], axis=1) - 1).max() <= 1e-12
    for key, n in (('vertices', nv - 1), ('faces', nf - 1)):
        short = dict(res, **{key: res[key][:, :n]})
        with pytest.raises(_lib.GnrError, match='max_' + key):
            mesh_from_extraction(short, 0)


# ---- write_ply (no GPU) --------------------------------------------------------------------------------------------------------
PLY_TODAY = ('ply\nformat ascii 1.0\ncomment graspnerf_amd surface cloud\nelement vertex 2\nproperty double x\nproperty double y\n'
             'property double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n'
             '0.0 0.0075 0.015 0 0 255\n0.2925 0.1 0.3333333333333333 64 128 255\n')


def test_write_ply_with_and_without_faces(tmp_path):
    path = os.path.join(str(tmp_path), 'mesh.ply')
    write_ply(path, np.array([[0.0, 0.0075, 0.015], [0.2925, 0.1, 1.0 / 3.0]]), [[0, 0, 1], [0.25, 0.5, 1.0]], faces=None)
    assert open(path, 'rb').read() == PLY_TODAY.encode()                        # without faces: byte for byte the format before them
    m = ref.surface_mesh(ref.sphere(*SPHERES[0]), scale=0.3 / 40, origin=(0.1, -0.2, 0.05))
    nv, nf = len(m['vertices']), len(m['faces'])
    col = np.linspace(0.0, 1.0, nv * 3).reshape(nv, 3)
    write_ply(path, m['vertices'], col, faces=m['faces'])
    lines = open(path).read().splitlines()
    end = lines.index('end_header')
    assert lines[:end] == ['ply', 'format ascii 1.0', 'comment graspnerf_amd surface cloud', f'element vertex {nv}', 'property double x',
                           'property double y', 'property double z', 'property uchar red', 'property uchar green', 'property uchar blue',
                           f'element face {nf}', 'property list uchar int vertex_indices']
    assert len(lines) == end + 1 + nv + nf
    rows = [l.split() for l in lines[end + 1:end + 1 + nv]]
    assert np.array_equal(np.array([[float(x) for x in r[:3]] for r in rows]), m['vertices'])       # repr round-trips float64
    assert np.array_equal(np.array([[int(x) for x in r[3:]] for r in rows]), np.floor(col * 255.0 + 0.5).astype(np.int64))
    tri = np.array([[int(x) for x in l.split()] for l in lines[end + 1 + nv:]])
    assert (tri[:, 0] == 3).all() and np.array_equal(tri[:, 1:], m['faces'])
    nrm = m['vertices'] / np.linalg.norm(m['vertices'], axis=1, keepdims=True)
    write_ply(path, m['vertices'], col, normals=nrm, faces=m['faces'])
    lines = open(path).read().splitlines()
    end = lines.index('end_header')
    assert lines[end - 2:end] == [f'element face {nf}', 'property list uchar int vertex_indices'] and 'property double nz' in lines[:end]
    assert np.array_equal(np.array([[float(x) for x in l.split()[3:6]] for l in lines[end + 1:end + 1 + nv]]), nrm)
    assert lines[end + 1 + nv:] == [f'3 {i} {j} {k}' for i, j, k in m['faces'].tolist()]
    with pytest.raises(ValueError):
        write_ply(path, m['vertices'], col, faces=[[0, 1, nv]])


# ---- GPU: the bits of the statement --------------------------------------------------------------------------------------------
R16 = 16
FRAME = dict(scale=0.3 / 40, origin=(0.125, -0.3, 0.0517))


def _shapes16():
    rng = np.random.default_rng(16)
    return np.stack([ref.sphere(R16, (7.3, 7.6, 7.45), 5.2), ref.torus(*TORUS), ref.plane(R16), rng.standard_normal((R16, R16, R16)).astype(np.float32)])


@pytest.fixture(scope='module')
def batch16():
    """The B = 4 batch at R = 16 with a random gradient volume, and the statement's mesh of every scene (computed once)."""
    vol = _shapes16()
    grad = np.random.default_rng(17).standard_normal((4, R16, R16, R16, 3)).astype(np.float32)
    want = [ref.surface_mesh(vol[b], iso=0.0, gradient=grad[b], **FRAME) for b in range(4)]
    return vol, grad, want


def _equal_scene(res, b, want, what, gradient=True):
    nv, nf = (int(c) for c in res['count'][b].tolist())
    assert (nv, nf) == (len(want['vertices']), len(want['faces'])), (what, 'counts', nv, nf)
    got = mesh_from_extraction(res, b)
    assert same(got['vertices'], want['vertices']), (what, 'vertices')
    assert same(got['faces'].astype(np.int32), want['faces']), (what, 'faces')
    if gradient:
        assert same(got['gradient'], want['gradient']), (what, 'gradient')
    return nv, nf


@pytest.mark.gpu
def test_batch_equals_the_statement_and_the_per_scene_calls(batch16):
    vol, grad, want = batch16
    ex = MeshExtractor()
    res = ex(vol, iso=0.0, gradient=grad, **FRAME)
    assert res['count'].shape == (4, 2) and res['vertices'].dtype == torch.float64 and res['faces'].dtype == torch.int32
    assert tuple(res['vertices'].shape[1:]) == (mesh_bounds(R16)[0], 3) and tuple(res['faces'].shape[1:]) == (mesh_bounds(R16)[1], 3)
    for b in range(4):
        nv, nf = _equal_scene(res, b, want[b], f'batched scene {b}')
        assert nv > 0 and nf > 0
        one = ex(vol[b], iso=0.0, gradient=grad[b:b + 1], **FRAME)
        _equal_scene(one, 0, want[b], f'scene {b} alone')
    plain = ex(vol, iso=0.0, **FRAME)                                             # without the gradient: the same mesh, no gradient rows
    assert 'gradient' not in plain
    for b in range(4):
        _equal_scene(plain, b, want[b], f'no gradient, scene {b}', gradient=False)
    m = mesh_from_extraction(res, 0)
    assert ref.signed_volume(m['vertices'], m['faces']) > 0 and np.abs(np.linalg.norm(m['normals'], axis=1) - 1).max() <= 1e-12


@pytest.mark.gpu
def test_iso_of_one_half_on_a_grid_in_the_unit_interval():
    rng = np.random.default_rng(5)
    vol = np.stack([(ref.sphere(R16, (7.3, 7.6, 7.45), 5.2) / 16 + 0.5).clip(0, 1), rng.random((R16, R16, R16)).astype(np.float32)]).astype(np.float32)
    vol[1, 3, 4, 5] = vol[1, 8, 8, 8] = 0.5                                       # equal to iso
    grad = rng.standard_normal((2, R16, R16, R16, 3)).astype(np.float32)
    res = MeshExtractor()(vol, iso=0.5, gradient=grad, **FRAME)
    for b in range(2):
        nv, _ = _equal_scene(res, b, ref.surface_mesh(vol[b], iso=0.5, gradient=grad[b], **FRAME), f'iso 0.5, scene {b}')
        assert nv > 0


@pytest.mark.gpu
@pytest.mark.parametrize('R', [2, 3, 5, 33, 34])
def test_sizes_at_which_the_compaction_can_go_wrong(R):
    """One cell and no interior edge; less than one wavefront of cells; 32^3 cells = exactly 32 chunks; 33^3, a ragged last chunk."""
    rng = np.random.default_rng(R)
    vol = rng.standard_normal((2, R, R, R)).astype(np.float32)
    if R == 2:
        vol[0] = 1.0
        vol[0, 1, 0, 1] = -0.25                                                   # scene 0: the one cell is active
    grad = rng.standard_normal((2, R, R, R, 3)).astype(np.float32)
    res = MeshExtractor()(vol, gradient=grad, **FRAME)
    for b in range(2):
        nv, nf = _equal_scene(res, b, ref.surface_mesh(vol[b], gradient=grad[b], **FRAME), f'R = {R}, scene {b}')
        if R == 2:
            assert nf == 0
    assert int(res['count'][0, 0]) > 0


@pytest.mark.gpu
def test_more_chunks_than_the_scan_has_threads():
    """R = 104: 1 068 chunks of cells and 1 099 of voxels per scene, so the scan of the chunk counts takes a second pass with a carried
    base; two scenes (the second one's offsets start from zero again)."""
    R = 104
    vol = np.stack([ref.sphere(R, (50.3, 51.6, 52.45), 47.0), ref.sphere(R, (52.3, 50.6, 51.45), 44.5)])
    res = MeshExtractor()(vol, **FRAME)
    for b in range(2):
        nv, nf = _equal_scene(res, b, ref.surface_mesh(vol[b], **FRAME), f'R = {R}, scene {b}', gradient=False)
        assert nv > 20000 and nf > 40000


def _raw(vol, max_v, max_f, grad=None, iso=0.0, sentinel=0x5a, slack=0):
    """The C call on buffers filled with a sentinel byte -> numpy count, vertices, faces, gradient (whole buffers).  slack (one scene
    only): rows allocated behind max_v / max_f that the call is not told about."""
    L = _lib.lib()
    B, R = vol.shape[0], vol.shape[-1]
    assert slack == 0 or B == 1
    AV, AF = max_v + slack, max_f + slack
    d = torch.device('cuda:0')
    v = torch.from_numpy(np.ascontiguousarray(vol)).to(d)
    g = None if grad is None else torch.from_numpy(np.ascontiguousarray(grad)).to(d)
    fill = lambda n, dt: torch.full((n,), sentinel, dtype=torch.uint8, device=d).view(dt)
    count = fill(B * 2 * 4, torch.int32)
    verts, faces = fill(B * AV * 3 * 8, torch.float64), fill(B * AF * 3 * 4, torch.int32)
    gout = None if grad is None else fill(B * AV * 3 * 4, torch.float32)
    ws = torch.full((L.gnr_surface_mesh_workspace_bytes(B, R),), 0xa7, dtype=torch.uint8, device=d)
    p = _lib.GnrMeshParams(iso=iso, scale=FRAME['scale'])
    p.origin[:] = FRAME['origin']
    rc = L.gnr_surface_mesh_fwd(v.data_ptr(), None if g is None else g.data_ptr(), B, R, C.byref(p), count.data_ptr(), verts.data_ptr(),
                                faces.data_ptr(), None if g is None else gout.data_ptr(), max_v, max_f, ws.data_ptr(), ws.numel(),
                                C.c_void_p(torch.cuda.current_stream(d).cuda_stream))
    _lib.check(rc, 'gnr_surface_mesh_fwd')
    torch.cuda.synchronize()
    return (count.cpu().numpy().reshape(B, 2), verts.cpu().numpy().reshape(B, AV, 3), faces.cpu().numpy().reshape(B, AF, 3),
            None if grad is None else gout.cpu().numpy().reshape(B, AV, 3))


def _untouched(a, sentinel=0x5a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == sentinel).all())


@pytest.mark.gpu
def test_empty_and_full_scenes_between_two_others(batch16):
    vol, grad, want = batch16
    v = np.stack([vol[0], np.full_like(vol[0], 0.75), np.full_like(vol[0], -0.75), vol[3]])
    g = np.stack([grad[0], grad[1], grad[2], grad[3]])
    MV, MF = mesh_bounds(R16)
    count, verts, faces, gout = _raw(v, MV, MF, grad=g)
    assert count[1].tolist() == [0, 0] and count[2].tolist() == [0, 0]
    for b in (1, 2):
        assert _untouched(verts[b]) and _untouched(faces[b]) and _untouched(gout[b])
    for b, w in ((0, want[0]), (3, want[3])):
        nv, nf = len(w['vertices']), len(w['faces'])
        assert count[b].tolist() == [nv, nf]
        assert same(verts[b, :nv], w['vertices']) and same(faces[b, :nf], w['faces']) and same(gout[b, :nv], w['gradient'])
        assert _untouched(verts[b, nv:]) and _untouched(faces[b, nf:]) and _untouched(gout[b, nv:])


@pytest.mark.gpu
def test_caps_keep_the_totals_and_store_the_prefix(batch16):
    vol, grad, want = batch16
    w = want[3]
    nv, nf = len(w['vertices']), len(w['faces'])
    assert nf % 2 == 0
    for MV, MF in ((nv - 1, nf), (nv, nf - 1)):                                   # (nf - 1 is odd: the last quad keeps its first triangle)
        count, verts, faces, gout = _raw(vol[3:4], MV, MF, grad=grad[3:4], slack=3)        # three rows behind the cap that the call does not know of
        assert count[0].tolist() == [nv, nf], 'count holds the totals beyond the caps'
        assert same(verts[0, :MV], w['vertices'][:MV]) and same(faces[0, :MF], w['faces'][:MF]) and same(gout[0, :MV], w['gradient'][:MV])
        assert _untouched(verts[0, MV:]) and _untouched(faces[0, MF:]) and _untouched(gout[0, MV:])
    ex = MeshExtractor()
    for kw, key in ((dict(max_vertices=nv - 1), 'max_vertices'), (dict(max_faces=nf - 1), 'max_faces')):
        res = ex(vol[3], gradient=grad[3:4], **FRAME, **kw)
        assert res['count'][0].tolist() == [nv, nf]
        with pytest.raises(_lib.GnrError, match=key):
            mesh_from_extraction(res, 0)
    # two scenes with a cap below both: neither writes into the other's rows
    MV, MF = 100, 151
    count, verts, faces, gout = _raw(vol[[3, 0]], MV, MF, grad=grad[[3, 0]])
    for b, s in ((0, 3), (1, 0)):
        kv, kf = min(MV, len(want[s]['vertices'])), min(MF, len(want[s]['faces']))
        assert count[b].tolist() == [len(want[s]['vertices']), len(want[s]['faces'])]
        assert same(verts[b, :kv], want[s]['vertices'][:kv]) and same(faces[b, :kf], want[s]['faces'][:kf])
        assert _untouched(verts[b, kv:]) and _untouched(faces[b, kf:])


@pytest.mark.gpu
def test_stale_workspace(batch16):
    vol, grad, want = batch16
    ex = MeshExtractor()
    dense = np.random.default_rng(34).standard_normal((1, 34, 34, 34)).astype(np.float32)
    big = ex(dense, **FRAME)
    assert int(big['count'][0, 0]) > 30000
    ex._ws.fill_(0x71)
    ws = ex._ws.data_ptr()
    res = ex(vol[0], gradient=grad[0:1], **FRAME)
    assert ex._ws.data_ptr() == ws                                                # the same, larger, workspace
    fresh = MeshExtractor()(vol[0], gradient=grad[0:1], **FRAME)
    _equal_scene(res, 0, want[0], 'stale workspace')
    _equal_scene(fresh, 0, want[0], 'fresh extractor')


@pytest.mark.gpu
def test_graph_capture_and_replay(batch16):
    vol, grad, want = batch16
    ex = MeshExtractor()
    d = ex.device
    static_v = torch.from_numpy(vol[1:2].copy()).to(d)
    static_g = torch.from_numpy(grad[1:2].copy()).to(d)
    s = torch.cuda.Stream(d)
    s.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(s):
        ex(static_v, gradient=static_g, **FRAME)                                  # the workspace exists before the capture
    torch.cuda.current_stream(d).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ex(static_v, gradient=static_g, **FRAME)
    for b in (0, 3):
        static_v.copy_(torch.from_numpy(vol[b:b + 1]))
        static_g.copy_(torch.from_numpy(grad[b:b + 1]))
        g.replay()
        torch.cuda.synchronize()
        _equal_scene(out, 0, want[b], f'replay with scene {b}')
        eager = MeshExtractor()(vol[b], gradient=grad[b:b + 1], **FRAME)
        nv, nf = eager['count'][0].tolist()
        assert same(out['vertices'][0, :nv].cpu().numpy(), eager['vertices'][0, :nv].cpu().numpy())
        assert same(out['faces'][0, :nf].cpu().numpy(), eager['faces'][0, :nf].cpu().numpy())
        assert same(out['gradient'][0, :nv].cpu().numpy(), eager['gradient'][0, :nv].cpu().numpy())


# ---- the real-robot route --------------------------------------------------------------------------------------------------------
def test_session_arguments_are_checked_before_anything_is_built():
    from graspnerf_amd import grasp_post
    with pytest.raises(TypeError, match='unknown mesh parameters'):
        grasp_post.mesh_params(dict(level=0.0))
    assert grasp_post.mesh_params(False) is None and grasp_post.mesh_params(True) == dict(iso=0.0, max_vertices=None, max_faces=None)
    assert grasp_post.mesh_params(dict(iso=0.25, max_faces=7)) == dict(iso=0.25, max_vertices=None, max_faces=7)


@pytest.mark.gpu
def test_plan_real_with_the_mesh_eager_and_session():
    """The synthetic checkpoint's volume need not cross zero (tests/test_planner_session.py:40): the level of the meshes that are compared
    is the eager volume's own median, and mesh=True (iso = 0) is compared with the statement whatever it holds."""
    from graspnerf_amd import planner
    from graspnerf_amd.synth import ring_cameras
    from test_planner_session import CFG, _state_dict
    from test_planner_session_real import V, HW, TOP_K, R, _frames
    net = planner.load_model(dict(CFG), {'network_state_dict': _state_dict(width_bias=5.0)})
    K = np.float32([[0.7 * HW[1], 0, 0.5 * HW[1]], [0, 0.7 * HW[1], 0.5 * HW[0]], [0, 0, 1]])
    cam = dict(extrinsics=list(ring_cameras(V)), intrinsic=K)
    A, B = _frames(1), _frames(2)
    vol = planner.plan_real(net, A, **cam)[2]
    rg = (float(np.percentile(vol, 40)), float(np.percentile(vol, 60)))
    iso = float(np.float32(np.median(vol)))
    kw = dict(order='score', top_k=TOP_K, surface_rg=rg, normals=True)
    plain = planner.plan_real(net, A, **cam, **kw, mesh=False)
    assert 'mesh' not in plain[3]
    eager = planner.plan_real(net, A, **cam, **kw, mesh=dict(iso=iso))
    sess = planner.real_session(net, V, HW, HW[::-1], order='score', top_k=TOP_K, surface_rg=rg, normals=True, mesh=dict(iso=iso))
    assert sess.captures == 1 and sess._d_out.numel() == 1 + 9 * sess.max_grasps + 1 + 2
    got = planner.plan_real(net, A, **cam, **kw, mesh=dict(iso=iso), session=sess)
    other = planner.plan_real(net, B, **cam, **kw, mesh=dict(iso=iso), session=sess)
    again = planner.plan_real(net, A, **cam, **kw, mesh=dict(iso=iso), session=sess)
    assert sess.captures == 1
    for what, res in (('eager', eager), ('session', got), ('session, second replay', again)):
        for k in ('index', 'pos', 'quat', 'width', 'score'):
            assert same(res[0][k], plain[0][k]), (what, k)                         # grasps, scores and cloud do not depend on the mesh
        assert same(res[1], plain[1]) and same(res[2], plain[2]), what
        for k in ('index', 'points', 'colors', 'gradient', 'normals'):
            assert same(res[3][k], plain[3][k]), (what, 'cloud', k)
        # ... and the mesh is the statement's on the returned volume, in the cloud's frame
        m = res[3]['mesh']
        want = ref.surface_mesh(res[2], iso=iso, scale=planner.REAL_VOXEL_SIZE)
        assert same(m['vertices'], want['vertices']), what
        assert m['faces'].dtype == np.int64 and np.array_equal(m['faces'], want['faces']), what
        assert same(m['gradient'], eager[3]['mesh']['gradient']) and same(m['normals'], eager[3]['mesh']['normals']), what
        assert len(m['vertices']) > 100 and len(m['faces']) > 100 and m['gradient'].shape == m['vertices'].shape
        # it overlays the cloud: every vertex lies inside the grid in the cloud's units
        assert m['vertices'].min() >= 0 and m['vertices'].max() <= (R - 1) * planner.REAL_VOXEL_SIZE
    mo = other[3]['mesh']
    wo = ref.surface_mesh(other[2], iso=iso, scale=planner.REAL_VOXEL_SIZE)
    assert same(mo['vertices'], wo['vertices']) and np.array_equal(mo['faces'], wo['faces']) and not same(other[2], got[2])
    # mesh=True: iso = 0
    zero = planner.plan_real(net, A, **cam, **kw, mesh=True)[3]['mesh']
    wz = ref.surface_mesh(plain[2], iso=0.0, scale=planner.REAL_VOXEL_SIZE)
    assert same(zero['vertices'], wz['vertices']) and np.array_equal(zero['faces'], wz['faces'])
    # a session without the option records what it records today and refuses a plan that asks for the mesh
    today = planner.real_session(net, V, HW, HW[::-1], order='score', top_k=TOP_K, surface_rg=rg, normals=True)
    assert today.mesh_params is None and 'mesh' not in today._out and today._d_out.numel() == 1 + 9 * today.max_grasps + 1
    t = planner.plan_real(net, A, **cam, **kw, session=today)
    assert 'mesh' not in t[3] and today.mesh is None
    with pytest.raises(ValueError, match='real_session'):
        planner.plan_real(net, A, **cam, **kw, session=today, mesh=True)
    with pytest.raises(ValueError, match='real_session'):
        planner.plan_real(net, A, **cam, **kw, session=sess, mesh=True)            # another level than the session's
