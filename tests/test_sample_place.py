"""Placement of the ordered samples by chunks (csrc/gnr_sample_order.h "the placement by chunks", k_sample_order).

The permutation of a render pass is defined by the host twin `gnr_sample_order_host`: perm[slot_of(start[key_i] + #{ j < i : key_j ==
key_i })] = i.  The device kernel places a scene's samples chunk by chunk, every chunk from the keys alone (the scene's histogram, the
histogram of the keys in front of the chunk, the rank inside the chunk), so:

* CPU: `gnr_sample_order_host_chunked`, the same chunk arithmetic run serially on the host, equals the host twin entry for entry, for
  every chunk size -- before the kernel ever runs;
* GPU: `gnr_debug_sample_order` (the launch the render passes make) equals the host twin around the kernel's chunk size, with different
  keys in every scene, twice with the same bytes, and at the largest sample count it accepts."""
import ctypes as C

import numpy as np
import pytest
import torch

from graspnerf_amd import _lib, weights

CHUNK = 4096                        # SO_CHUNK of csrc/gnr_kernels.hip: samples a workgroup of k_sample_order places
MAX_SORT_SAMPLES = 1 << 18


def host_order(keys):
    keys = np.ascontiguousarray(keys, np.uint8)
    perm = np.full(len(keys), -1, np.int32)
    _lib.check(_lib.lib().gnr_sample_order_host(keys.ctypes.data_as(C.c_void_p), len(keys), perm.ctypes.data_as(C.c_void_p)), 'gnr_sample_order_host')
    return perm


def host_order_chunked(keys, chunk):
    keys = np.ascontiguousarray(keys, np.uint8)
    perm = np.full(len(keys), -1, np.int32)
    _lib.check(_lib.lib().gnr_sample_order_host_chunked(keys.ctypes.data_as(C.c_void_p), len(keys), chunk, perm.ctypes.data_as(C.c_void_p)),
               'gnr_sample_order_host_chunked')
    return perm


def key_arrays(P, rng):
    rnd = rng.integers(0, 256, P).astype(np.uint8)
    return {'one constant key': np.full(P, 0x2d, np.uint8),
            'two alternating keys': np.where(np.arange(P) % 2 == 0, 0x15, 0x3e).astype(np.uint8),
            'all 256 values cycling': (np.arange(P) % 256).astype(np.uint8),
            'random bytes': rnd,
            'random 6-bit masks': rng.integers(0, 64, P).astype(np.uint8),
            'sorted ascending': np.sort(rnd),
            'sorted descending': np.sort(rnd)[::-1].copy()}


@pytest.mark.parametrize('P', [1, 5, 16, 17, 143, 1023, 1024, 1025, 2049, 20480, 20481])
def test_the_chunked_placement_is_the_host_twin(P):
    """(tests/golden/maskstat_cfg2_fine_depth.npz holds the fine DEPTHS of the cfg2 scenes, not their keys: no case from it.)"""
    rng = np.random.default_rng(7000 + P)
    for name, keys in key_arrays(P, rng).items():
        want = host_order(keys)
        assert np.array_equal(np.sort(want), np.arange(P)), name
        for chunk in (64, 256, 1024, 4096):
            assert np.array_equal(host_order_chunked(keys, chunk), want), (name, chunk)


def test_the_chunked_host_twin_checks_its_arguments():
    keys, perm = np.zeros(4, np.uint8), np.zeros(4, np.int32)
    L = _lib.lib()
    kp, pp = keys.ctypes.data_as(C.c_void_p), perm.ctypes.data_as(C.c_void_p)
    assert L.gnr_sample_order_host_chunked(kp, 4, 0, pp) != 0
    assert L.gnr_sample_order_host_chunked(kp, 0, 64, pp) != 0
    assert L.gnr_sample_order_host_chunked(None, 4, 64, pp) != 0
    assert L.gnr_sample_order_host_chunked(kp, 4, 64, pp) == 0


# ---------------------------------------------------------------------------------------------------------------- GPU
def _hp(wnp):
    from graspnerf_amd.hotpath import HotPath
    return HotPath(weights.pack_state_dict(wnp, 'coarse'), weights.pack_state_dict(wnp, 'fine'))


@pytest.mark.gpu
@pytest.mark.parametrize('P', [1, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 17, 20480])
def test_three_scenes_with_their_own_keys(P, weights_np):
    """B = 3, a different key array per scene (a workgroup that reads another scene's keys gets another permutation; scene b starts b * P
    bytes behind an aligned address, so for P not a multiple of 16 scenes 1 and 2 start inside a 16-byte word of the kernel's counting
    loads): every row is the host twin's, and a second launch on the same keys returns the same bytes."""
    hp = _hp(weights_np)
    rng = np.random.default_rng(9000 + P)
    arrays = [np.full(P, 0x2d, np.uint8), (np.arange(P) % 256).astype(np.uint8), rng.integers(0, 256, P).astype(np.uint8)]
    keys = torch.from_numpy(np.stack(arrays)).cuda()
    perm = hp.debug_sample_order(keys)
    again = hp.debug_sample_order(keys)
    assert torch.equal(perm, again)
    perm = perm.cpu().numpy()
    for b, k in enumerate(arrays):
        assert np.array_equal(perm[b], host_order(k)), f'scene {b}'


@pytest.mark.gpu
@pytest.mark.parametrize('offset', [1, 7, 15])
def test_a_scene_that_starts_inside_a_word(offset, weights_np):
    """B = 1, the keys `offset` bytes behind an aligned address and CHUNK + 1 of them: the first and the last 16-byte word of the counting
    loads hold bytes in front of and behind the scene (here 0xff fill, which must not be counted)."""
    hp = _hp(weights_np)
    P = CHUNK + 1
    keys = np.random.default_rng(offset).integers(0, 64, P).astype(np.uint8)
    buf = torch.full((P + 32,), 0xff, dtype=torch.uint8, device='cuda')
    buf[offset:offset + P] = torch.from_numpy(keys).cuda()
    view = buf[offset:offset + P].view(1, P)
    assert view.data_ptr() % 16 == offset
    perm = hp.debug_sample_order(view).cpu().numpy()
    assert np.array_equal(perm[0], host_order(keys))


@pytest.mark.gpu
def test_the_largest_scene(weights_np):
    """B = 1, P = 2^18 (MAX_SORT_SAMPLES: 64 chunks, each counting all 2^18 keys) of random 6-bit masks against the host twin."""
    hp = _hp(weights_np)
    keys = np.random.default_rng(18).integers(0, 64, MAX_SORT_SAMPLES).astype(np.uint8)
    perm = hp.debug_sample_order(torch.from_numpy(keys[None])).cpu().numpy()
    assert np.array_equal(perm[0], host_order(keys))
