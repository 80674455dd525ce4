"""ST section of the packed forward blob (csrc/gnr_layout.h): the K-stacked fp16-pair fragments of ray_dir_fc.2, rgb_fc.2 and of
rgb_fc.0's k-steps 8, 9, which the pair instantiations of k_chain (inference and training forward) multiply on
v_mfma_f32_16x16x32_f16.  No GPU.

A stacked layer puts its SLOTS = 4 (2) real inputs per lane into the k-slots of ONE K32 block next to the residual terms of the
unscaled pair form (x = h + m, s = h 2^-11, w = wh + wm 2^-11):
    SLOTS 4:  A {wh0..3, wm0..3} x B {h0..3, s0..3}, then A x B {m0..3, 0, 0, 0, 0}
    SLOTS 2:  A {wh, wm, wh, wm} x B {h0, h1, s0, s1, m0, m1, 0, 0}
Emulated here from the section's bytes with the ISA lane mapping (A[i = l & 15][k = 8 (l >> 4) + e], B[k][j = l & 15]): fp16
operands, exact products, one fp32 rounding of the accumulator per MFMA; compared with the dense float64 layer under the bound
tests/test_pack_layout.py::test_pair_fragments uses for the K32 pair layers (3e-7 of sum|w x|)."""
import numpy as np
import pytest

from graspnerf_amd import weights
from graspnerf_amd.synth import synth_state_dict
from test_pack_layout import LAYERS, LOG2E, bias_acc, emulate, from_D, nat, off, to_B

PAIR_BOUND = 3e-7          # test_pack_layout.py::test_pair_fragments
SPEC = {l[0]: l for l in LAYERS}


def _other_seed(weights_np):
    """The same tensors drawn from another seed (synth.synth_state_dict: N(0, 1 / fan_in) weights)."""
    return synth_state_dict({k: v.shape for k, v in weights_np.items()}, seed=23)


@pytest.fixture(scope='module', params=['seed0', 'seed23'])
def packed_and_sd(request, weights_np):
    sd = weights_np if request.param == 'seed0' else _other_seed(weights_np)
    return weights.pack_state_dict(sd, 'coarse'), sd


def split_unscaled(x):
    """fp32 [..] -> (h, m, s) as float64 values of fp16 numbers: h = fp16(x), m = fp16(x - h), s = fp16(h 2^-11)."""
    x = x.astype(np.float32)
    h = x.astype(np.float16)
    m = (x - h.astype(np.float32)).astype(np.float16)
    s = h * np.float16(1.0 / 2048.0)
    return h.astype(np.float64), m.astype(np.float64), s.astype(np.float64)


def stacked_halfs(packed, name, SLOTS, NB):
    """-> wh, wm [NB][64 lanes][SLOTS] (float64 values of the stored halfs)."""
    raw = packed[off(name): off(name) + NB * 64 * SLOTS].view(np.float16).reshape(NB, 64, 2, SLOTS).astype(np.float64)
    return raw[:, :, 0], raw[:, :, 1]


def mfma(A, B, acc):
    """One v_mfma_f32_16x16x32_f16: A [64 lanes][8], B [64 lanes][8] (fp16 values), acc [4][64] fp32 -> fp32."""
    out = np.empty_like(acc)
    for l in range(64):
        col = l & 15
        for t in range(4):
            i = 4 * (l >> 4) + t
            out[t, l] = np.float32(acc[t, l] + sum(np.dot(A[i + 16 * k], B[col + 16 * k]) for k in range(4)))
    return out


def emulate_stacked(packed, name, SLOTS, NB, Bin, acc):
    """Bin [SLOTS][64] fp32 inputs of the lanes -> acc [NB][4][64] += W x as mm16s computes it."""
    wh, wm = stacked_halfs(packed, name, SLOTS, NB)
    h, m, s = (v.T for v in split_unscaled(Bin))                     # [64][SLOTS]
    z = np.zeros_like(h)
    out = acc.astype(np.float32).copy()
    for nb in range(NB):
        if SLOTS == 4:
            A = np.concatenate([wh[nb], wm[nb]], 1)
            out[nb] = mfma(A, np.concatenate([h, s], 1), out[nb])
            out[nb] = mfma(A, np.concatenate([m, z], 1), out[nb])
        else:
            A = np.concatenate([wh[nb], wm[nb], wh[nb], wm[nb]], 1)
            out[nb] = mfma(A, np.concatenate([h, s, m, z], 1), out[nb])
    return out.astype(np.float64)


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def test_stacked_four_slot_layers(packed_and_sd):
    """ray_dir_fc.2 (16 -> 35 in the x layout, three output blocks) and rgb_fc.2 (16 -> 8): inputs are scaled-ELU outputs."""
    packed, sd = packed_and_sd
    for lname, sname, seed in (('rdf2', 'ST_RDF2', 31), ('rgb2', 'ST_RGB2', 32)):
        _, _, (bname, badd), J, NB, key, phi, psi, iscale, oscale = SPEC[lname]
        assert J == 4
        W, b = sd[key + '.weight'], sd[key + '.bias']
        x = elu(2.0 * np.random.default_rng(seed).standard_normal((16, W.shape[1]))).astype(np.float32)     # bounded below, a few units above
        xk = (x * np.array([iscale(i) for i in range(W.shape[1])])).astype(np.float32)
        acc = emulate_stacked(packed, sname, 4, NB, to_B(xk, 4, phi), bias_acc(packed, off('C16.' + bname) + badd, NB))
        y = from_D(acc, NB, psi, W.shape[0])
        ref = oscale * (x.astype(np.float64) @ W.T.astype(np.float64) + b)
        mag = oscale * (np.abs(x.astype(np.float64)) @ np.abs(W.T.astype(np.float64)) + np.abs(b))
        assert np.max(np.abs(y - ref) / mag) < PAIR_BOUND, lname
        # same slots, same rows as the fp32 fragment it replaces (the next layer's B layout does not move)
        y32 = from_D(emulate(packed, off(SPEC[lname][1][0]), 4, NB, to_B(xk, 4, phi), bias_acc(packed, off(bname) + badd, NB)), NB, psi, W.shape[0])
        np.testing.assert_allclose(y, y32, rtol=0, atol=2e-6 * float(mag.max()))


def test_stacked_two_slot_extras_of_rgb_fc0(packed_and_sd):
    """rgb_fc.0's inputs 32..36 (vis2 in [0, 1], the direction difference |.| <= 2 and the cosine): k-steps 8 and 9 of the layer,
    all three partial products in one MFMA."""
    packed, sd = packed_and_sd
    _, _, _, J, NB, key, phi, psi, iscale, oscale = SPEC['rgb1']
    W = sd[key + '.weight'].astype(np.float64)
    rng = np.random.default_rng(33)
    d = rng.standard_normal((2, 16, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    x = np.zeros((16, 37), np.float32)
    x[:, 32] = rng.random(16)
    x[:, 33:36] = d[0] - d[1]
    x[:, 36] = (d[0] * d[1]).sum(-1)
    Bin = to_B(x, 10, phi)[8:10]                                      # true scale: iscale(i >= 32) == 1
    assert iscale(32) == 1.0
    acc = emulate_stacked(packed, 'ST_RGB1X', 2, 1, Bin, np.zeros((1, 4, 64)))
    y = from_D(acc, 1, psi, 16)
    ref = oscale * (x[:, 32:].astype(np.float64) @ W[:, 32:].T)
    mag = oscale * (np.abs(x[:, 32:].astype(np.float64)) @ np.abs(W[:, 32:].T))
    assert np.max(np.abs(y - ref) / mag) < PAIR_BOUND


def test_the_c16_image_keeps_its_fp32_fragments(packed_and_sd):
    """The section sits in front of the C16 image; the image itself is what it was: ray_dir_fc and rgb_fc.2 as copies of the fp32
    fragments, rgb_fc.0's two left-over k-steps behind its K32 block (tests/test_pack_layout.py pins the image's layout; k_chain
    stages the stacked fragments over these ranges of its LDS copy)."""
    packed, _ = packed_and_sd
    assert off('ST_RDF2') == off('RM_END') and off('ST_END') == off('C16')
    assert (off('ST_RGB2') - off('ST_RDF2'), off('ST_RGB1X') - off('ST_RGB2'), off('ST_END') - off('ST_RGB1X')) == (768, 256, 128)
    assert off('TOTAL') == off('C16') + off('C16_END')
    assert np.array_equal(packed[off('C16.RDF1'): off('C16.NR1')], packed[off('RDF1'): off('NR1')])
    assert np.array_equal(packed[off('C16.RGB2'): off('C16.HOIST')], packed[off('RGB2'): off('HOIST')])
    assert np.array_equal(packed[off('C16.RGB1') + 512: off('C16.RGB2')], packed[off('RGB1') + 512: off('RGB2')])
    assert np.isfinite(packed[off('ST_RDF2'): off('ST_END')].view(np.float16).astype(np.float32)).all()
    assert packed[off('T_VIS') + 2] == 0.0 and packed[off('C16.T_VIS') + 2] == 0.0


@pytest.mark.parametrize('key,sec,n', [('ray_dir_fc.2', 'ST_RDF2', 768), ('rgb_fc.2', 'ST_RGB2', 256), ('rgb_fc.0', 'ST_RGB1X', 128)])
def test_a_weight_without_a_pair_is_inf_and_marks_the_blob(key, sec, n, weights_np):
    w = dict(weights_np)
    k = 'agg_net.agg_impl.' + key + '.weight'
    w[k] = w[k].copy()
    w[k][1, w[k].shape[1] - 1] = 1e6            # (rgb_fc.0: column 36, one of the stacked k-steps)
    p = weights.pack_state_dict(w, 'coarse')
    halfs = p[off(sec): off(sec) + n].view(np.float16)
    assert np.isinf(halfs).sum() == 1 and halfs[np.isinf(halfs)][0] > 0
    assert p[off('T_VIS') + 2] == 1.0 and p[off('C16.T_VIS') + 2] == 1.0
