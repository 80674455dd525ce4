"""Row-by-row check of the CPU oracle against the reference's own functions on random inputs.
The reference's outputs and the seeded inputs they were computed from are stored in tests/golden/golden_ref_ops.npz
(tools/make_goldens.py --ref-ops-only): the oracle is run on the stored inputs and compared with the stored outputs."""
import os

import numpy as np
import pytest
import torch

from oracle import graspnerf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def G():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_ref_ops.npz'))
    return {k: torch.from_numpy(g[k]) for k in g.files}


@pytest.mark.parametrize('seed', range(8))
def test_projection_rows_P1_P3(seed, G):
    g = lambda k: G[f'P.{seed}.{k}']
    pts, poses, Ks = g('pts'), g('poses'), g('Ks')
    H, W = (int(x) for x in g('hw'))
    rfn, N = poses.shape[0], pts.shape[0]
    uv, z, mask, dirv = O.project_points(pts, poses, Ks, H, W)
    uv_r, z_r, dir_r, mk = g('uv'), g('z'), g('dir'), g('mask')
    # same formula, different contraction order (einsum vs batched matmul): fp32 rounding only
    wc = z.reshape(rfn, N).abs() > 1e-2                        # u = x/z is ill-conditioned next to the camera plane
    assert torch.allclose(uv.reshape(rfn, N, 2)[wc], uv_r[wc], rtol=1e-4, atol=1e-3)
    assert torch.allclose(z.reshape(rfn, N), z_r, rtol=1e-6, atol=1e-7)
    assert torch.allclose(dirv, dir_r, atol=1e-6)
    u, v = uv[..., 0], uv[..., 1]
    marg = torch.minimum(torch.minimum((u + 0.5).abs(), (u - (W - 0.5)).abs()), torch.minimum((v + 0.5).abs(), (v - (H - 0.5)).abs()))
    safe = (marg > 1e-2) & wc
    assert torch.equal(mask.reshape(rfn, N)[safe], mk[safe]) and safe.float().mean() > 0.9


@pytest.mark.parametrize('seed', range(8))
def test_bilinear_row_I1(seed, G):
    g = lambda k: G[f'I.{seed}.{k}']
    h, w = (int(x) for x in g('hw'))
    got = O.bilinear_border(g('feat'), g('uv'), h, w)
    assert torch.allclose(got, g('out'), atol=2e-6, rtol=1e-5)


@pytest.mark.parametrize('seed', range(6))
def test_depth_sampling_rows_S1_S3_C0_F1(seed, G):
    g = lambda k: G[f'S.{seed}.{k}']
    rn, dn, fdn = (int(x) for x in g('shape'))
    dr, hp = g('dr'), g('hp')
    d = O.sample_depth(dr, rn, dn)
    assert torch.equal(d, g('depth'))
    assert torch.allclose(O.alpha_to_hit_prob(g('alpha')), g('hit'), atol=1e-7)
    fd, _ = O.sample_fine_depth(d, hp, dr, fdn)
    assert torch.allclose(fd, g('fine_det'), atol=1e-6)
    fd, _ = O.sample_fine_depth(d, hp, dr, fdn, u=g('u'))      # u: the uniform draw the reference's resampling made
    assert torch.allclose(fd, g('fine_rand'), atol=1e-6)
    lo, hi = O.ray_half_intervals(d, dr)
    base = (-1.0 - (-1.0)) / ((-0.5) - (-1.0))
    assert torch.allclose(base - g('near'), lo, atol=1e-7) and torch.allclose(g('far') - base, hi, atol=1e-7)


@pytest.mark.parametrize('seed', range(6))
def test_decoder_rows_D1_D3(seed, G, weights_np):
    g = lambda k: G[f'D.{seed}.{k}']
    f, z, dr = g('f'), g('z'), g('dr')
    V, N = z.shape
    W = {k: torch.from_numpy(v) for k, v in weights_np.items()}
    hit, vis = O.decode_hit_vis(W, 'dist_decoder.', f, z, torch.ones(V, N, dtype=torch.bool), dr, 0.005, 0.005)
    assert torch.allclose(hit, g('hit'), atol=2e-6) and torch.allclose(vis, g('vis'), atol=2e-6)


@pytest.mark.parametrize('seed', range(4))
def test_mean_variance_embedding_and_posenc_rows_A2_A3(seed, G):
    g = lambda k: G[f'A.{seed}.{k}']
    x, w = g('x'), g('w')
    m, v = O.weighted_mean_var(x.permute(2, 0, 1, 3).reshape(4, 45, 7), w.permute(2, 0, 1, 3).reshape(4, 45, 1))
    assert torch.allclose(m, g('mean'), atol=1e-6) and torch.allclose(v, g('var'), atol=1e-6)
    assert int(G['A.embed_dim']) == 21 and torch.equal(O.embed_points(g('p')), g('embed'))
    for n in (16, 40):
        assert torch.equal(O.sinusoid_table(n), G[f'A.pos{n}'])


def test_neus_alpha_row_N1(G, weights_np):
    g = lambda k: G[f'N.{k}']
    a = O.neus_alpha(g('sdf'), g('grad'), g('qdir'), g('depth'), torch.tensor(0.3))
    assert torch.allclose(a, g('alpha'), atol=1e-6)
