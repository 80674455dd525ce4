"""HIP grasp head (csrc/gnr_head.hip) vs the PyTorch fp32 ConvNet (backbone.ConvNet, itself bit-identical to the
reference's gd.networks.ConvNet on CPU: tests/test_model_mirror.py), and the inference kernels against a float64 statement of that
network at every kind of volume edge R the library accepts (8..64): both kernels behind decoder.conv1 / decoder.conv2 (LDS-staged up to
R = 40, direct gather from R = 41), odd edges in the stride-2 encoder, ragged nearest-neighbour maps d3 -> 10, every intermediate
activation, and the tails of the sigmoid and of F.normalize."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import PARITY_LOG, ROOT
from graspnerf_amd import _lib, grasp_head
from graspnerf_amd.backbone import ConvNet
from graspnerf_amd.synth import synth_state_dict


def _net():
    net = ConvNet().eval()
    syn = synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=11)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in syn.items()})
    return net


# ---- the float64 statement (gd/networks.py:39-97) and the gate ---------------------------------------------------------------------
TAPS = ('a1', 'a2', 'a3', 'a4', 'a5', 'a6')
OUTS = ('qual', 'rot', 'width')
LAYERS = [name for name, _ in grasp_head.HEAD_KEYS]
# (R, B): lower edge (d3 = 1) | odd everywhere | ragged 3 -> 10 | ragged 4 -> 10 | largest staged halo, odd | the planner's | first direct
# size, 3 x 27 = 81 bricks: the last workgroup holds one wavefront | ragged 7 -> 10 on the direct path | upper edge
SIZES = [(8, 1), (9, 3), (17, 1), (26, 1), (33, 1), (40, 2), (41, 3), (50, 1), (64, 1)]
RECORD = {}          # case -> {tensor: ratios}: head_fp64_arbiter.json in $GNR_RECORD_DIR when that is set (-> profiles/); PARITY_LOG always


def convnet_taps(sd, vol):
    """ConvNet.forward in the dtype of `vol`, from F.conv3d / F.relu / F.interpolate(size=10 / 20 / 40) alone: every post-ReLU activation
    (a1..a6), the three head pre-activations and the three outputs."""
    def conv(x, name, stride=1):
        w = sd[name + '.weight'].to(vol.dtype)
        return F.conv3d(x, w, sd[name + '.bias'].to(vol.dtype), stride=stride, padding=w.shape[-1] // 2)
    t = {}
    t['a1'] = F.relu(conv(vol, 'encoder.conv1', 2))
    t['a2'] = F.relu(conv(t['a1'], 'encoder.conv2', 2))
    t['a3'] = F.relu(conv(t['a2'], 'encoder.conv3', 2))
    t['a4'] = F.relu(conv(t['a3'], 'decoder.conv1'))
    t['a5'] = F.relu(conv(F.interpolate(t['a4'], size=10), 'decoder.conv2'))
    t['a6'] = F.relu(conv(F.interpolate(t['a5'], size=20), 'decoder.conv3'))
    x = F.interpolate(t['a6'], size=40)
    t['pre_qual'], t['pre_rot'], t['pre_width'] = conv(x, 'conv_qual'), conv(x, 'conv_rot'), conv(x, 'conv_width')
    t['qual'], t['rot'], t['width'] = torch.sigmoid(t['pre_qual']), F.normalize(t['pre_rot'], dim=1), t['pre_width']
    return t


def _weights(wset):
    sd = {k: v.clone() for k, v in _net().state_dict().items()}
    if wset == 'tails':                      # logits far into both tails of the sigmoid; F.normalize on its eps branch
        sd['conv_qual.weight'] *= 400.0
        sd['conv_rot.weight'].zero_()
        sd['conv_rot.bias'].zero_()
    else:
        assert wset == 'seed11'
    return sd


def _volume(R, B):
    return torch.rand(B, 1, R, R, R, generator=torch.Generator().manual_seed(R)) * 2 - 1


@functools.lru_cache(maxsize=None)
def _case(R, B, wset='seed11'):
    """Volume, weights and the CPU references (float64, float32) of one case: computed once, shared, never written to."""
    sd, vol = _weights(wset), _volume(R, B)
    with torch.no_grad():
        return {'sd': sd, 'vol': vol, 'f64': convnet_taps(sd, vol.double()), 'f32': convnet_taps(sd, vol)}


def _rms(x):
    return float(x.double().pow(2).mean().sqrt())


def gate_bounds(name, f64, f32):
    """The gate on one tensor, from the CPU references alone (no kernel enters): (rms bound, per-element max bound).
       rms(e) <= 3 rms(e_32) + floor,   |e| <= 3 max|e_32| + floor   with e_32 = torch fp32 - float64, floor = 2^-24 rms(float64 tensor)
    (half an fp32 ulp of the tensor's size: tests/test_bwd_arbiter.py; the factor 3 is the one the feature extractor's HIP glue is held
    to against ATen).  qual and rot get 4 fp32 ulp of the reference value per element on top, 4 x 2^-23 x |f64|, for their pointwise last
    step, which the conv's own error model does not cover.  From the CDNA3/CDNA4 instruction set references V_EXP_F32, V_RCP_F32 and V_SQRT_F32
    are accurate to 1 ulp, and hipcc rounds fp32 `/` and sqrtf correctly by default (0.5 ulp).  rot = x / max(sqrtf(x.x), eps): four squares and
    three adds (<= 2 ulp on the sum, 1 on its root), the root 0.5, the division 0.5: 2 ulp.  qual = 1 / (1 + __expf(-x)) with __expf(y) =
    v_exp_f32(y log2 e): the product's rounding is |x| / 2 ulp on e, the instruction 1, the sum 0.5, the division 0.5, so relative to qual
    (1 - q)(1.5 + |x| / 2) + 1 ulp: below 4 for |x| <= 4 and for every x > 4; for x < -4 it is q |x| / 2 ulp of 1.0 in absolute terms,
    < 0.04 x 2^-23, under the floor of any qual tensor with an rms above 0.1.  So 4 ulp stands as the issue set it."""
    e_32 = (f32.double() - f64).abs()
    floor = 2.0 ** -24 * _rms(f64)
    allow = 4 * 2.0 ** -23 * f64.abs() if name in ('qual', 'rot') else torch.zeros_like(f64)
    return 3 * _rms(e_32) + floor + _rms(allow), 3 * float(e_32.max()) + floor + allow


def _ratio(err, bound):
    """err / bound elementwise, worst element; 0 / 0 (both sides exact) counts as 0, anything / 0 as inf."""
    err, bound = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64)
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(q.max())


def _head_against_float64(R, B, wset):
    """Run the HIP head on the case, hold all nine tensors to the gate, record every ratio.  -> (outputs on the CPU, reference case)"""
    case = _case(R, B, wset)
    head = grasp_head.GraspHead(case['sd'])
    out = head(case['vol'].cuda())
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in head.activations(B, R).items()}
    got.update({k: v.cpu() for k, v in zip(OUTS, out)})
    rows, bad = {}, []
    for name in TAPS + OUTS:
        f64, f32 = case['f64'][name], case['f32'][name]
        assert got[name].shape == f64.shape and bool(torch.isfinite(got[name]).all()), name
        b_rms, b_max = gate_bounds(name, f64, f32)
        e_hip = (got[name].double() - f64).abs()
        size = _rms(f64)
        rows[name] = {'rms_ratio': _ratio(_rms(e_hip), b_rms), 'max_ratio': _ratio(e_hip, b_max),
                      'hip_rms_err_over_rms': _rms(e_hip) / size if size else 0.0,
                      'torch_fp32_rms_err_over_rms': _rms(f32.double() - f64) / size if size else 0.0}
        print(f'R={R} B={B} {wset} {name}: rms ratio {rows[name]["rms_ratio"]:.3f}  max ratio {rows[name]["max_ratio"]:.3f}  '
              f'(hip {rows[name]["hip_rms_err_over_rms"]:.2e}, torch fp32 {rows[name]["torch_fp32_rms_err_over_rms"]:.2e} of rms)')
        if not (rows[name]['rms_ratio'] <= 1.0 and rows[name]['max_ratio'] <= 1.0):
            bad.append((name, rows[name]))
    tag = f'R={R} B={B} {wset}'
    RECORD[tag] = rows
    worst = max(max(r['rms_ratio'], r['max_ratio']) for r in rows.values())
    PARITY_LOG.append({'what': f'grasp head fp64 arbiter, {tag}', 'ratios': rows, 'max_abs': max(r['hip_rms_err_over_rms'] for r in rows.values()),
                       'max_over_tol': worst})
    if os.environ.get('GNR_RECORD_DIR'):
        out = os.path.join(ROOT, os.environ['GNR_RECORD_DIR'])
        try:
            os.makedirs(out, exist_ok=True)
            json.dump(RECORD, open(os.path.join(out, 'head_fp64_arbiter.json'), 'w'), indent=1)
        except OSError:
            pass
    assert not bad, (tag, bad)          # the first tap in the list is the layer that went wrong
    return got, case


def test_pack_sizes_and_key_order():
    net = _net()
    blob = grasp_head.canonical_blob(net.state_dict())
    assert blob.size == sum(v.numel() for v in net.state_dict().values()) == _lib.lib().gnr_head_canonical_floats()
    packed = grasp_head.pack(blob)
    assert packed.size == _lib.lib().gnr_head_packed_floats() and np.isfinite(packed).all()
    # first layer keeps canonical order; fused heads: bias block order rot0..3, qual, width
    np.testing.assert_array_equal(packed[:2000], net.state_dict()['encoder.conv1.weight'].numpy().reshape(-1))
    sd = net.state_dict()
    hb = packed[-16:-10]
    np.testing.assert_array_equal(hb, np.concatenate([sd['conv_rot.bias'].numpy(), sd['conv_qual.bias'].numpy(), sd['conv_width.bias'].numpy()]))
    assert _lib.lib().gnr_pack_grasp_head(None, None) == -1


@pytest.mark.gpu
@pytest.mark.parametrize('R,B', [(40, 2), (16, 1)])
def test_head_matches_pytorch(R, B):
    """The module itself (backbone.ConvNet) as the fp32 reference, and the float64 gate of _head_against_float64 on top."""
    net = _net()
    vol = _volume(R, B)
    with torch.no_grad():
        q0, r0, w0 = net(vol)
    got, case = _head_against_float64(R, B, 'seed11')
    q, r, w = got['qual'], got['rot'], got['width']
    assert torch.equal(case['vol'], vol)
    assert q.shape == (B, 1, 40, 40, 40) and r.shape == (B, 4, 40, 40, 40) and w.shape == (B, 1, 40, 40, 40)
    np.testing.assert_allclose(q.numpy(), q0.numpy(), rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(w.numpy(), w0.numpy(), rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(r.numpy(), r0.numpy(), rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(np.linalg.norm(r.numpy(), axis=1), 1.0, atol=1e-5)     # unit quaternions


@pytest.mark.gpu
@pytest.mark.parametrize('R,B', SIZES)
def test_head_against_float64_at_every_kind_of_size(R, B):
    """All six activations and the three outputs within the gate (gate_bounds) at the nine sizes of SIZES, seed-11 weights, volume uniform
    in [-1, 1].  R <= 40 runs decoder.conv1 / conv2 on k_conv3d_staged, R >= 41 on k_conv3d_direct at stride 1 (conv2 through the index map)."""
    got, _ = _head_against_float64(R, B, 'seed11')
    np.testing.assert_allclose(np.linalg.norm(got['rot'].numpy(), axis=1), 1.0, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('R,B', [(33, 1), (41, 1)])
def test_head_against_float64_in_the_tails_of_the_epilogue(R, B):
    """conv_qual.weight x 400: the logits span both tails of the sigmoid (logits from -34 to +80: __expf of large arguments of either sign, quality from
    1e-15 up to exactly 1).  conv_rot all zero: F.normalize divides 0 by its eps, rot is exactly 0 on both sides."""
    got, case = _head_against_float64(R, B, 'tails')
    lo, hi = float(case['f64']['pre_qual'].min()), float(case['f64']['pre_qual'].max())
    assert lo < -17 and hi > 17, (lo, hi)                   # 1 - sigmoid(17) < 2^-24: fp32 saturates on both sides
    assert not case['f64']['rot'].any() and not case['f32']['rot'].any() and not got['rot'].any()
    assert float(got['qual'].min()) >= 0.0 and float(got['qual'].max()) <= 1.0


def _bits(ts):
    return [t.detach().cpu().contiguous().view(torch.int32) for t in ts]


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))


PROPERTY_SIZES = [(9, 3), (41, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize('R,B', PROPERTY_SIZES)
def test_a_batched_call_is_the_one_scene_calls(R, B):
    head, vol = grasp_head.GraspHead(_weights('seed11')), _volume(R, B).cuda()
    whole = head(vol)
    for b in range(B):
        assert _same_bits(head(vol[b:b + 1]), [t[b:b + 1] for t in whole]), b


@pytest.mark.gpu
@pytest.mark.parametrize('R,B', PROPERTY_SIZES)
def test_two_calls_return_the_same_bits(R, B):
    head, vol = grasp_head.GraspHead(_weights('seed11')), _volume(R, B).cuda()
    first = _bits(head(vol))
    assert _same_bits(first, head(vol))


@pytest.mark.gpu
@pytest.mark.parametrize('R,B', PROPERTY_SIZES)
def test_nothing_is_read_from_the_workspace_before_it_is_written(R, B):
    """The whole workspace (activations and index maps) filled with NaN before the call: no output bit changes."""
    head, vol = grasp_head.GraspHead(_weights('seed11')), _volume(R, B).cuda()
    first = _bits(head(vol))
    head._ws.view(torch.float32).fill_(float('nan'))
    assert _same_bits(first, head(vol))


@pytest.mark.gpu
@pytest.mark.parametrize('R,B', PROPERTY_SIZES)
def test_a_larger_workspace_left_by_another_size_changes_nothing(R, B):
    """One GraspHead called at R = 64 and then at this size keeps the larger workspace, full of the other size's activations and index map."""
    sd, vol = _weights('seed11'), _volume(R, B).cuda()
    fresh = _bits(grasp_head.GraspHead(sd)(vol))
    head = grasp_head.GraspHead(sd)
    head(_volume(64, B).cuda())
    n = head._ws.numel()
    assert n > _lib.lib().gnr_grasp_head_workspace_bytes(B, R)
    assert _same_bits(fresh, head(vol)) and head._ws.numel() == n


# ---- CPU: the packing, the index maps, the gate's teeth, the refusals ------------------------------------------------------------------
_CELL = ((-1, -1, 0, 0, 1), (-1, 0, 0, 1, 1))       # source cell of tap d - 2 behind a x2 nearest upsampling, output parity 0 / 1


def _unpack_fragments(frag, cout, cin, k):
    """[tap][cin / 4][cout blocks][64 lanes] -> dense [cout blocks x 16][cin][tap]: lane & 15 = output channel in the block, lane >> 4 =
    input channel mod 4."""
    nb = (cout + 15) // 16
    f = frag.reshape(k ** 3, cin // 4, nb, 4, 16)               # [tap][c][nb][g][r]
    return f.transpose(2, 4, 1, 3, 0).reshape(nb * 16, cin, k ** 3)


def _fold_float64(w):
    """[co][ci][5][5][5] -> [8 parity classes][co][ci][27]: the tap sums of a k5 conv behind a x2 nearest upsampling as a k3 conv on the
    source grid, accumulated in float64 in tap order and rounded once to fp32."""
    w = w.astype(np.float64)
    out = np.zeros((8,) + w.shape[:2] + (3, 3, 3))
    for par in range(8):
        pz, py, px = (par >> 2) & 1, (par >> 1) & 1, par & 1
        for dz in range(5):
            for dy in range(5):
                for dx in range(5):
                    out[par, :, :, _CELL[pz][dz] + 1, _CELL[py][dy] + 1, _CELL[px][dx] + 1] += w[:, :, dz, dy, dx]
    return out.astype(np.float32).reshape(8, w.shape[0], w.shape[1], 27)


def _equal_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_fragment_round_trip():
    """gnr_pack_grasp_head's blob unpacked back to dense weights: the plain layers bit for bit, padded lanes exactly 0, the biases in
    their stated order, the two folded layers equal to the float64 tap sums rounded once."""
    sd = {k: v.numpy() for k, v in _net().state_dict().items()}
    packed = grasp_head.pack(grasp_head.canonical_blob(sd))
    off = 0

    def take(n):
        nonlocal off
        off += n
        return packed[off - n:off]
    assert _equal_bits(take(2000), sd['encoder.conv1.weight'].reshape(-1)) and _equal_bits(take(16), sd['encoder.conv1.bias'])
    for name, (co, ci, k) in grasp_head.HEAD_KEYS[1:5]:
        w = _unpack_fragments(take(27 * (ci // 4) * (co // 16) * 64), co, ci, k)
        assert _equal_bits(w, sd[name + '.weight'].reshape(co, ci, 27)), name
        assert _equal_bits(take(co), sd[name + '.bias']), name
    # decoder.conv3: 8 parity classes x 27 taps, 32 -> 16
    want = _fold_float64(sd['decoder.conv3.weight'])
    for par in range(8):
        assert _equal_bits(_unpack_fragments(take(27 * 8 * 64), 16, 32, 3), want[par]), par
    assert _equal_bits(take(16), sd['decoder.conv3.bias'])
    # the fused heads, 16 -> 6 padded to 16 lanes, channel order rot0..3, qual, width
    hw = np.concatenate([sd['conv_rot.weight'], sd['conv_qual.weight'], sd['conv_width.weight']])
    want = _fold_float64(hw)
    assert want.shape == (8, 6, 16, 27)
    for par in range(8):
        w = _unpack_fragments(take(27 * 4 * 64), 6, 16, 3)
        assert _equal_bits(w[:6], want[par]), par
        assert not w[6:].view(np.int32).any(), par                  # padded lanes: +0.0, not a small number and not -0.0
    hb = take(16)
    assert _equal_bits(hb[:6], np.concatenate([sd['conv_rot.bias'], sd['conv_qual.bias'], sd['conv_width.bias']])) and not hb[6:].view(np.int32).any()
    assert off == packed.size == _lib.lib().gnr_head_packed_floats()
    # the fold itself: each of the 125 taps lands in exactly one cell, so every class sums to the plain k5 weight sum
    np.testing.assert_allclose(want.astype(np.float64).sum(-1), np.broadcast_to(hw.astype(np.float64).sum((2, 3, 4)), (8, 6, 16)), rtol=0, atol=1e-5)


def test_activation_layout_is_the_librarys_workspace():
    for R in range(8, 65):
        for B in (1, 3):
            layout = grasp_head.activation_layout(B, R)                 # asserts total + 4096 == gnr_grasp_head_workspace_bytes
            assert [n for n, _, _ in layout] == list(TAPS)
            assert all(o1 == o0 + int(np.prod(s0)) for (_, o0, s0), (_, o1, _) in zip(layout, layout[1:]))
    d = [s[2] for _, _, s in grasp_head.activation_layout(3, 41)]
    assert d == [21, 11, 6, 6, 10, 20] and grasp_head.activation_layout(3, 41)[2][2] == (3, 64, 6, 6, 6)
    for B, R in [(1, 7), (1, 65), (0, 40)]:
        with pytest.raises(ValueError):
            grasp_head.activation_layout(B, R)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_nearest_index_maps(dtype):
    """What k_umaps has to reproduce: F.interpolate(size=10) from an edge of d = 1..8 picks source i * d // 10 on every axis, and the fixed
    10 -> 20 and 20 -> 40 maps pick i // 2, in float32 and in float64."""
    for d, n in [(d, 10) for d in range(1, 9)] + [(10, 20), (20, 40)]:
        want = torch.arange(n) * d // n
        if n != 10:
            assert torch.equal(want, torch.arange(n) // 2)
        for axis in (2, 3, 4):
            shape = [1, 1, 1, 1, 1]
            shape[axis] = d
            x = torch.arange(d, dtype=dtype).view(shape).expand(1, 1, d, d, d).contiguous()
            y = F.interpolate(x, size=n).movedim(axis, -1)[0, 0, 0, 0]
            assert torch.equal(y.long(), want), (d, n, axis)


def test_the_gate_has_teeth():
    """One weight (w[0,0,0,0,0]) of each of the nine layers set to zero, in the float64 statement alone, at R = 41, B = 1: every such
    mutation moves at least one output by at least 10 x the gate's rms bound (which comes from the fp32 evaluation and from no kernel)."""
    case = _case(41, 1)
    bound = {name: gate_bounds(name, case['f64'][name], case['f32'][name])[0] for name in OUTS}
    vol64 = case['vol'].double()
    factors = {}
    for layer in LAYERS:
        sd = dict(case['sd'])
        sd[layer + '.weight'] = sd[layer + '.weight'].clone()
        sd[layer + '.weight'][0, 0, 0, 0, 0] = 0.0
        with torch.no_grad():
            mut = convnet_taps(sd, vol64)
        factors[layer] = max(_rms(mut[name] - case['f64'][name]) / bound[name] for name in OUTS)
        print(f'{layer}: w[0,0,0,0,0] = 0 moves an output by {factors[layer]:.1f} x the gate')
    assert min(factors.values()) >= 10, factors


def test_head_refuses_bad_shapes_before_touching_a_device():
    L = _lib.lib()
    one = C.c_void_p(16)                                    # never dereferenced: the argument checks come first
    big = C.c_size_t(1 << 40)

    def call(B, R, vol=one, ws=one, ws_bytes=big):
        return L.gnr_grasp_head_fwd(B, R, vol, one, one, one, one, ws, ws_bytes, None)
    for B, R in [(1, 7), (1, 65), (0, 40)]:
        assert call(B, R) == _lib.GNR_ERR_SHAPE and b'bad B/R' in L.gnr_head_last_error(), (B, R)
    assert call(1, 40, vol=None) == _lib.GNR_ERR_ARG and b'null pointer' in L.gnr_head_last_error()
    assert call(1, 40, ws=None) == _lib.GNR_ERR_ARG and b'null pointer' in L.gnr_head_last_error()
    for B, R in [(1, 8), (3, 41), (1, 64)]:
        short = C.c_size_t(L.gnr_grasp_head_workspace_bytes(B, R) - 1)
        assert call(B, R, ws_bytes=short) == _lib.GNR_ERR_WORKSPACE and b'workspace too small' in L.gnr_head_last_error(), (B, R)


@pytest.mark.gpu
@pytest.mark.parametrize('B,Cin,Cout,D,H,W,K', [(2, 16, 6, 9, 7, 10, 5), (1, 32, 16, 6, 6, 6, 5), (3, 20, 33, 5, 4, 7, 3), (1, 16, 6, 40, 40, 40, 5)])
def test_conv3d_same_all_three_directions(B, Cin, Cout, D, H, W, K):
    """conv3d_same under autograd = gnr_conv3d_same (forward, backward data) + gnr_conv3d_same_bwd_weight against PyTorch's own
    conv3d forward / backward (ragged channel counts incl. several 16-channel chunks, non-cubic volumes that are not
    multiples of the 8x8x4 brick)."""
    from graspnerf_amd.backbone import conv3d_same
    g = torch.Generator().manual_seed(B * 100 + Cin)
    x = torch.randn(B, Cin, D, H, W, generator=g).cuda().requires_grad_(True)
    w = (0.1 * torch.randn(Cout, Cin, K, K, K, generator=g)).cuda().requires_grad_(True)
    b = torch.randn(Cout, generator=g).cuda().requires_grad_(True)
    dy = torch.randn(B, Cout, D, H, W, generator=g).cuda()
    y = conv3d_same(x, w, b)
    (y * dy).sum().backward()
    got = (y.detach().clone(), x.grad.clone(), w.grad.clone(), b.grad.clone())
    x.grad = w.grad = b.grad = None
    y0 = torch.nn.functional.conv3d(x, w, b, padding=K // 2)
    (y0 * dy).sum().backward()
    for a, r, name in zip(got, (y0.detach(), x.grad, w.grad, b.grad), ('y', 'dx', 'dw', 'db')):
        assert a.shape == r.shape and (a - r).abs().max() <= 2e-4 * r.abs().max() + 1e-5, name


def test_folded_upsample_k5_is_the_plain_convolution():
    """backbone.upconv5_x2 = F.conv3d(F.interpolate(u, x2 nearest), w, b, padding=2) in values and in all three gradients (float64 on
    the CPU, ragged sizes: the fold is exact algebra, the zero padding of the upsampled grid included)."""
    from graspnerf_amd import backbone
    import torch.nn.functional as F
    torch.manual_seed(3)
    u = torch.randn(2, 5, 6, 4, 7, dtype=torch.float64, requires_grad=True)
    w = torch.randn(3, 5, 5, 5, 5, dtype=torch.float64, requires_grad=True)
    b = torch.randn(3, dtype=torch.float64, requires_grad=True)
    saved = dict(backbone._FOLD_MATS)
    try:
        backbone._FOLD_MATS.clear()
        backbone._FOLD_MATS[('up', 'cpu')] = backbone._upfold_matrix('cpu').double()
        y = backbone.upconv5_x2(u, w, b)
    finally:
        backbone._FOLD_MATS.clear(); backbone._FOLD_MATS.update(saved)
    r = F.conv3d(F.interpolate(u, scale_factor=2, mode='nearest'), w, b, padding=2)
    assert y.shape == r.shape and float((y - r).abs().max()) < 1e-12
    g = torch.randn_like(r)
    for a, c in zip(torch.autograd.grad((y * g).sum(), (u, w, b)), torch.autograd.grad((r * g).sum(), (u, w, b))):
        assert float((a - c).abs().max()) < 1e-11


@pytest.mark.parametrize('k,ci,co,dims', [(3, 4, 5, (6, 4, 8)), (5, 1, 3, (8, 6, 4)), (5, 2, 3, (4, 4, 4)), (3, 3, 2, (2, 2, 2))])
def test_stride2_as_space_to_depth_is_the_plain_convolution(k, ci, co, dims):
    """backbone.conv3d_stride2 = F.conv3d(x, w, b, stride=2, padding=k // 2) in values and all three gradients (float64, CPU)."""
    from graspnerf_amd import backbone
    import torch.nn.functional as F
    torch.manual_seed(k + ci)
    x = torch.randn(2, ci, *dims, dtype=torch.float64, requires_grad=True)
    w = torch.randn(co, ci, k, k, k, dtype=torch.float64, requires_grad=True)
    b = torch.randn(co, dtype=torch.float64, requires_grad=True)
    saved = dict(backbone._FOLD_MATS)
    try:
        backbone._FOLD_MATS.clear()
        backbone._FOLD_MATS[(k, 'cpu')] = backbone._stride2_matrix(k, 'cpu').double()
        y = backbone.conv3d_stride2(x, w, b)
    finally:
        backbone._FOLD_MATS.clear(); backbone._FOLD_MATS.update(saved)
    r = F.conv3d(x, w, b, stride=2, padding=k // 2)
    assert y.shape == r.shape and float((y - r).abs().max()) < 1e-12
    g = torch.randn_like(r)
    for a, c in zip(torch.autograd.grad((y * g).sum(), (x, w, b)), torch.autograd.grad((r * g).sum(), (x, w, b))):
        assert float((a - c).abs().max()) < 1e-11


@pytest.mark.gpu
@pytest.mark.parametrize('k,ci,co,n,B', [(5, 1, 16, 40, 2), (3, 16, 32, 20, 2), (3, 32, 64, 10, 3), (3, 20, 24, 6, 1), (5, 3, 5, 8, 2)])
def test_stride2_layers_on_the_hip_path(k, ci, co, n, B):
    """The encoder's stride-2 layers (gd/networks.py:33-37) as space-to-depth + masked k3 convolution (gnr_conv3d_same_masked,
    gnr_conv3d_same_bwd_weight_masked: taps without a weight skipped per 16 x 16 channel block) against F.conv3d(stride=2): outputs
    and all three gradients.  Some weights are set to exactly 0.0: the mask is structure, their gradients must still come out."""
    from graspnerf_amd import backbone
    import torch.nn.functional as F
    torch.manual_seed(k * 100 + ci)
    x = torch.randn(B, ci, n, n, n, device='cuda', requires_grad=True)
    w = (torch.randn(co, ci, k, k, k, device='cuda') * 0.2)
    w[:, :, 0] = 0.0
    w[: co // 2, :, :, 1] = 0.0
    w.requires_grad_(True)
    b = torch.randn(co, device='cuda', requires_grad=True)
    y = backbone.conv3d_stride2(x, w, b)
    r = F.conv3d(x, w, b, stride=2, padding=k // 2)
    assert y.shape == r.shape and float((y - r).detach().abs().max()) <= 2e-5 * float(r.detach().abs().max())
    g = torch.randn_like(r)
    ga = torch.autograd.grad((y * g).sum(), (x, w, b))
    gr = torch.autograd.grad((r * g).sum(), (x, w, b))
    for name, a, c in zip(('dx', 'dw', 'db'), ga, gr):
        assert float((a - c).abs().max()) <= 1e-4 * float(c.abs().max()) + 1e-6, name
    assert float(ga[1][:, :, 0].abs().max()) > 0                      # a gradient where the weight's VALUE is zero


@pytest.mark.gpu
@pytest.mark.parametrize('masked', [False, True])
def test_k3_kernel_generations_agree(masked):
    """The pipelined K = 3 kernels (k_conv3d_s1_k3 / k_conv3d_wgrad_k3: buffer loads, register prefetch) against the first-generation
    ones they replace (kept for volumes beyond 32-bit byte offsets; GNR_CONV3D_FIRST_GEN per call): same products in the same order per
    output, so forward and backward data agree to rounding of the MFMA chain and the weight gradient to 1e-5 of its scale."""
    from graspnerf_amd import backbone, _lib
    L = _lib.lib()
    torch.manual_seed(5)
    if masked:
        x = torch.randn(2, 16, 20, 20, 20, device='cuda', requires_grad=True)
        w = (torch.randn(32, 16, 3, 3, 3, device='cuda') * 0.1).requires_grad_(True)
        f = lambda: backbone.conv3d_stride2(x, w, b)
    else:
        x = torch.randn(2, 40, 9, 10, 11, device='cuda', requires_grad=True)
        w = (torch.randn(24, 40, 3, 3, 3, device='cuda') * 0.1).requires_grad_(True)
        f = lambda: backbone.conv3d_same(x, w, b)
    b = torch.randn(w.shape[0], device='cuda', requires_grad=True)
    res = []
    for gen in (0, 1):
        prev, backbone.CONV3D_FIRST_GEN = backbone.CONV3D_FIRST_GEN, bool(gen)
        try:
            y = f()
            g = torch.autograd.grad((y * torch.cos(y.detach())).sum(), (x, w))
            torch.cuda.synchronize()
        finally:
            backbone.CONV3D_FIRST_GEN = prev
        res.append((y.detach(), g[0], g[1]))
    for a, c in zip(*res):
        assert float((a - c).abs().max()) <= 1e-5 * float(c.abs().max()) + 1e-7


@pytest.mark.gpu
def test_convnet_under_autograd_matches_pytorch():
    """gd.networks.ConvNet mirror in training mode (HIP convolutions; decoder.conv3 and the fused heads with their x2 upsampling
    folded into pre-summed k3 weights, backbone.upconv5_x2; the encoder's stride-2 layers as space-to-depth + k3, backbone.conv3d_stride2) against the same module stated plainly in PyTorch (F.interpolate +
    F.conv3d, no folding): outputs and all 18 parameter gradients."""
    from graspnerf_amd import backbone
    torch.manual_seed(0)
    net = backbone.ConvNet().cuda()
    vol = torch.randn(2, 1, 40, 40, 40, device='cuda').clamp(-1, 1)
    ups = [torch.randn(2, c, 40, 40, 40, device='cuda') for c in (1, 4, 1)]
    res = {}
    for hip in (True, False):
        net.zero_grad(set_to_none=True)
        orig, fold, s2d = backbone.conv3d_same, backbone.FOLD_UPSAMPLED_K5, backbone.STRIDE2_AS_S2D
        if not hip:
            backbone.conv3d_same = lambda x, w, b: torch.nn.functional.conv3d(x, w, b, padding=w.shape[-1] // 2)
            backbone.FOLD_UPSAMPLED_K5 = backbone.STRIDE2_AS_S2D = False
        try:
            out = net(vol)
            sum((o * u).sum() for o, u in zip(out, ups)).backward()
        finally:
            backbone.conv3d_same, backbone.FOLD_UPSAMPLED_K5, backbone.STRIDE2_AS_S2D = orig, fold, s2d
        torch.cuda.synchronize()
        res[hip] = ([o.detach().clone() for o in out], {k: p.grad.clone() for k, p in net.named_parameters()})
    for a, r in zip(res[True][0], res[False][0]):
        assert (a - r).abs().max() <= 1e-4 * r.abs().max() + 1e-6
    for k, r in res[False][1].items():
        assert (res[True][1][k] - r).abs().max() <= 5e-4 * r.abs().max() + 1e-6, k


@pytest.mark.gpu
@pytest.mark.parametrize('B,Cin,Cout,D,H,W,K', [(2, 16, 6, 9, 7, 10, 5), (1, 40, 20, 6, 5, 9, 3)])
def test_first_generation_weight_gradient_kernel(B, Cin, Cout, D, H, W, K):
    """gnr_conv3d_bwd_weight (any odd K; kept in the ABI) against PyTorch."""
    import ctypes as C
    from graspnerf_amd import _lib
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, Cin, D, H, W, generator=g).cuda()
    dy = torch.randn(B, Cout, D, H, W, generator=g).cuda()
    dw = torch.zeros(Cout, Cin, K, K, K, device='cuda')
    assert _lib.lib().gnr_conv3d_bwd_weight(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, Cin, Cout, D, H, W, K, None) == 0
    want = torch.nn.grad.conv3d_weight(x, dw.shape, dy, padding=K // 2)
    torch.cuda.synchronize()
    assert (dw - want).abs().max() <= 2e-4 * want.abs().max() + 1e-5
