"""The binned scatter of the feature-map gradient (csrc/gnr_bwd_scatter.inc) as a stage of its own.

The view kernel parks one 64-value row per (view, point) with a bin key (scene-view * npix + top-left tap pixel, -1 = dead) and four
tap weights; k_scatter_place -- or k_scatter_scan + k_scatter_fill above 38 400 pixels -- lists the rows bin by bin, k_scatter_gather
sums them per pixel (the right-hand pixels' sums ride along to the next bin), k_unpack_feat_grad turns the channel-last buffer into
NCHW.  Whole backwards reach this code at 1e-3 of a tensor's maximum; here it runs alone (gnr_debug_feature_scatter) against

* a float64 numpy model of the stage, per output entry, at a bound derived from the arithmetic (float mode), and
* an integer model of the fixed-point mode, bit for bit,

both written from the comments of the .inc files.  Further down: the product's threshold between the two placements end to end
(part B), and a range-flagged pass on a poisoned workspace (part C: the scatter kernels consume nothing the view kernel did not park).

CPU (no marker): the models against a brute-force loop and under a permutation of the rows."""
import numpy as np
import pytest

# ---- the reference ----------------------------------------------------------------------------------------------------------------
# position of a value in a parked row -> channel: the lane of point r, group g stores its 8 ray-feature and its 8 image-feature
# gradients as 16 consecutive floats at 16 g (ray channels 8 g + j, image channels 32 + 8 g + j)
CHANNEL = np.array([8 * (p // 16) + p % 16 if p % 16 < 8 else 32 + 8 * (p // 16) + (p % 16 - 8) for p in range(64)])
TAPS = ((0, 0), (0, 1), (1, 0), (1, 1))          # (dy, dx) of w00 w01 w10 w11


def _tap_targets(key, wts, fh, fw):
    """Per tap: (rows that contribute, their flat entry index / 64).  A row contributes to a tap when it is live, the tap's weight is
    not zero and the tap exists: in the last column / row the far taps are skipped whatever they weigh."""
    npix = fh * fw
    o = np.where(key >= 0, key % npix, 0)
    y0, x0 = o // fw, o % fw
    for t, (dy, dx) in enumerate(TAPS):
        ok = (key >= 0) & (wts[:, t] != 0)
        if dx:
            ok &= x0 < fw - 1
        if dy:
            ok &= y0 < fh - 1
        idx = np.nonzero(ok)[0]
        yield t, idx, key[idx].astype(np.int64) + dy * fw + dx


def model_float64(rows, wts, key, BV, fh, fw):
    """-> (sum [BV, npix, 64] float64, n = contributions per entry, S = sum of their absolute values)."""
    npix = fh * fw
    out, n, S = (np.zeros((BV * npix, 64), dt) for dt in (np.float64, np.int64, np.float64))
    for t, idx, pix in _tap_targets(key, wts, fh, fw):
        c = np.zeros((len(idx), 64))
        c[:, CHANNEL] = rows[idx].astype(np.float64) * wts[idx, t].astype(np.float64)[:, None]
        np.add.at(out, pix, c)
        np.add.at(S, pix, np.abs(c))
        np.add.at(n, pix, 1)
    return out.reshape(BV, npix, 64), n.reshape(BV, npix, 64), S.reshape(BV, npix, 64)


def fx_exponent(upmax):
    """e with 2^e > upmax (finite, > 0), clamped to [-90, 100]; 0 otherwise."""
    mx = np.float32(upmax)
    if not (mx > 0) or not (mx < np.float32(3.0e38)):
        return 0
    return int(max(min(np.frexp(mx)[1], 100), -90))


def model_fixed(rows, wts, key, BV, fh, fw, upmax):
    """The fixed-point mode: every contribution rounded once to a multiple of the quantum 2^(e - 28), summed as integers.
    -> (values [BV, npix, 64] float32, integer sums, clamped: bit 3)."""
    npix = fh * fw
    e = fx_exponent(upmax)
    scale = np.float32(2.0) ** np.float32(28 - e)
    acc = np.zeros((BV * npix, 64), np.int64)
    clamped = False
    for t, idx, pix in _tap_targets(key, wts, fh, fw):
        with np.errstate(over='ignore', invalid='ignore'):
            y = (rows[idx].astype(np.float32) * wts[idx, t].astype(np.float32)[:, None]).astype(np.float32) * scale      # float32 product, then x 2^k
        over = ~(np.abs(y) < np.float32(2.0 ** 42))
        if over.any():
            clamped = True
            y = np.where(over, np.where(np.isnan(y), np.float32(0), np.copysign(np.float32(2.0 ** 42), y)), y)
        q = np.zeros((len(idx), 64), np.int64)
        q[:, CHANNEL] = np.rint(y.astype(np.float64)).astype(np.int64)                # ties to even
        np.add.at(acc, pix, q)
    val = (acc.astype(np.float64) * 2.0 ** (e - 28)).astype(np.float32)
    return val.reshape(BV, npix, 64), acc.reshape(BV, npix, 64), clamped


def to_nchw(chan_last, B, V, fh, fw):
    """[BV, npix, 64] -> d_ray_feats, d_img_feats [B, V, 32, fh, fw]"""
    a = chan_last.reshape(B, V, fh, fw, 64).transpose(0, 1, 4, 2, 3)
    return a[:, :, :32], a[:, :, 32:]


# ---- the generator ----------------------------------------------------------------------------------------------------------------
def make_rows(rng, pix, fh, fw, regime, zero_tap_every=7):
    """pix [B, V, cap] (pixel of the row's top-left tap inside its scene-view, -1 = dead; cap a multiple of 16) -> rows [N, 64],
    wts [N, 4], key [N] in the stage's row order ((b * tps + tile) * V + v) * 16 + point.  Bilinear weights; a row in the last
    column / row carries zero far weights (the stage's precondition, make_taps); every few rows one more tap is zero."""
    B, V, cap = pix.shape
    tps, npix = cap // 16, fh * fw
    seg = (np.arange(B)[:, None] * V + np.arange(V)[None])[..., None]
    k = np.where(pix >= 0, seg * npix + pix, -1)                                        # [B, V, cap]
    key = k.reshape(B, V, tps, 16).transpose(0, 2, 1, 3).reshape(-1).astype(np.int32)
    N = key.size
    o = np.where(key >= 0, key % npix, 0)
    y0, x0 = o // fw, o % fw
    fx, fy = rng.uniform(0.05, 0.95, N), rng.uniform(0.05, 0.95, N)
    fx[x0 == fw - 1] = 0.0
    fy[y0 == fh - 1] = 0.0
    z = np.arange(N) % zero_tap_every == 0
    fx[z] = 0.0
    wts = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], -1).astype(np.float32)
    if regime == 'normal':
        rows = rng.standard_normal((N, 64))
    else:                                                                               # magnitudes spread over 1e-6 .. 1e3
        rows = 10.0 ** rng.uniform(-6, 3, (N, 64)) * rng.choice([-1.0, 1.0], (N, 64))
    return rows.astype(np.float32), wts, key


def _pix(B, V, cap, fill=-1):
    return np.full((B, V, cap), fill, np.int64)


def case_pixels(name, rng):
    """-> (B, V, fh, fw, pix [B, V, cap]).  The smallest shapes that reach each branch of placement and gather."""
    if name == 'cap16 3x3 every pixel':                       # below one chunk; four corners, last column, last row; npix < 1024
        p = _pix(1, 2, 16)
        p[0, 0] = np.concatenate([np.arange(9), rng.integers(0, 9, 7)])
        p[0, 1, :9] = np.arange(9)[::-1]                      # a descending run parked, listed ascending; 7 dead rows behind it
        return 1, 2, 3, 3, p
    if name == 'cap80 dead rows interleaved':
        p = _pix(1, 2, 80)
        p[0, 0] = rng.integers(0, 9, 80)
        p[0, 0, ::3] = -1
        p[0, 1] = rng.integers(0, 9, 80)
        p[0, 1, 1::2] = -1
        return 1, 2, 3, 3, p
    if name == 'cap128 bin ends at entry 64':                 # pixel 0 holds list entries 0 .. 63 exactly, pixel 1 starts the second chunk
        p = _pix(1, 2, 128)
        p[0, 0] = rng.permutation(np.concatenate([np.zeros(64, np.int64), np.ones(40, np.int64), rng.integers(2, 9, 24)]))
        p[0, 1] = rng.permutation(np.concatenate([np.full(64, 4), np.full(64, 5)]))       # ... and ends at the list's end
        return 1, 2, 3, 3, p
    if name == 'cap144 one pixel':                            # one bin cut by two chunk boundaries
        p = _pix(1, 2, 144)
        p[0, 0] = 4
        p[0, 1] = 8                                           # the bottom-right corner: no far tap at all
        return 1, 2, 3, 3, p
    if name == 'raster run 40x30':                            # consecutive keys: every step carries, except across the line ends
        p = _pix(1, 2, 144)
        p[0, 0] = 3 * 40 + np.arange(144)                     # lines 3 .. 6: crosses three line ends
        p[0, 1, :16] = 7 * 40 + 5 + np.arange(16)             # a run inside one line; 128 dead rows behind it
        return 1, 2, 30, 40, p
    if name == 'line end 40x30':                              # (y, fw - 1) then (y + 1, 0): consecutive keys that must not carry
        p = _pix(1, 2, 16)
        p[0, 0, :4] = [5 * 40 + 39, 6 * 40, 5 * 40 + 39, 6 * 40]
        p[0, 1, :6] = [39, 40, 29 * 40 + 39, 28 * 40 + 39, 29 * 40 + 38, 29 * 40]      # corners and the ends of the first / last line
        return 1, 2, 30, 40, p
    if name == 'borders 40x30':                               # four corners, whole last column, whole last row, 1200 pixels (not a multiple of 1024)
        p = _pix(1, 2, 80)
        p[0, 0, :30] = np.arange(30) * 40 + 39
        p[0, 0, 30:70] = 29 * 40 + np.arange(40)
        p[0, 0, 70:74] = [0, 39, 29 * 40, 29 * 40 + 39]
        p[0, 1] = rng.integers(0, 1200, 80)
        return 1, 2, 30, 40, p
    if name == 'B3 V3 empty segment between live ones':       # scene-view 4 has no live row (nseg = 0), scene-view 5 has every row live
        p = rng.integers(0, 9, (3, 3, 32))
        p[rng.random(p.shape) < 0.3] = -1
        p[1, 1] = -1
        p[1, 2] = rng.integers(0, 9, 32)
        return 3, 3, 3, 3, p
    if name == 'B2 V8 32x32':                                 # 1024 pixels: every scan thread owns exactly one
        p = rng.integers(0, 1024, (2, 8, 48))
        p[..., :8] = rng.integers(0, 4, (2, 8, 8)) + 1020     # ... and the last threads' pixels are hit
        p[rng.random(p.shape) < 0.25] = -1
        return 2, 8, 32, 32, p
    raise KeyError(name)


CASES = ['cap16 3x3 every pixel', 'cap80 dead rows interleaved', 'cap128 bin ends at entry 64', 'cap144 one pixel', 'raster run 40x30',
         'line end 40x30', 'borders 40x30', 'B3 V3 empty segment between live ones', 'B2 V8 32x32']
REGIMES = ['normal', 'wide']


def make_case(name, regime):
    rng = np.random.default_rng([CASES.index(name), REGIMES.index(regime)])
    B, V, fh, fw, pix = case_pixels(name, rng)
    rows, wts, key = make_rows(rng, pix, fh, fw, regime)
    return B, V, fh, fw, pix.shape[2] // 16, rows, wts, key


def shuffle_inside_pairs(rng, rows, wts, key):
    """Another order of the 16 rows of every (tile, view): each row keeps its key and its weights."""
    n = key.size // 16
    perm = (np.arange(n)[:, None] * 16 + np.argsort(rng.random((n, 16)), 1)).reshape(-1)
    return rows[perm], wts[perm], key[perm]


# ---- CPU: the models' self-test ---------------------------------------------------------------------------------------------------
def _brute_force(rows, wts, key, BV, fh, fw):
    out = np.zeros((BV, fh * fw, 64))
    for i in range(key.size):
        if key[i] < 0:
            continue
        seg, o = divmod(int(key[i]), fh * fw)
        y0, x0 = divmod(o, fw)
        for pos in range(64):
            g, j = divmod(pos, 16)
            ch = 8 * g + j if j < 8 else 32 + 8 * g + j - 8
            for (dy, dx), w in zip(TAPS, wts[i]):
                if y0 + dy < fh and x0 + dx < fw:
                    out[seg, (y0 + dy) * fw + x0 + dx, ch] += float(rows[i, pos]) * float(w)
    return out


@pytest.mark.parametrize('name', ['cap16 3x3 every pixel', 'cap80 dead rows interleaved'])
def test_float64_model_is_the_brute_force_loop(name):
    B, V, fh, fw, tps, rows, wts, key = make_case(name, 'normal')
    got, n, S = model_float64(rows, wts, key, B * V, fh, fw)
    want = _brute_force(rows, wts, key, B * V, fh, fw)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    assert (got[n == 0] == 0).all() and (S >= np.abs(got) * (1 - 1e-12)).all()
    assert n.max() > 4
    live = key >= 0
    assert n[..., 0].sum() == sum(len(idx) for _, idx, _ in _tap_targets(key, wts, fh, fw)) <= 4 * live.sum()
    # every key lies in its own row's scene-view range (the generator's promise to the GPU tests)
    seg = (np.arange(key.size) // 16) % V + (np.arange(key.size) // (16 * V * tps)) * V
    assert ((key[live] // (fh * fw)) == seg[live]).all()


def test_generator_respects_the_precondition():
    for name in CASES:
        B, V, fh, fw, tps, rows, wts, key = make_case(name, 'wide')
        assert key.size == B * tps * V * 16 and rows.shape == (key.size, 64)
        o = np.where(key >= 0, key % (fh * fw), 0)
        assert (wts[o % fw == fw - 1][:, [1, 3]] == 0).all() and (wts[o // fw == fh - 1][:, [2, 3]] == 0).all()
        assert np.isfinite(rows).all() and np.abs(rows[rows != 0]).min() > 1e-7          # far from denormals


@pytest.mark.parametrize('regime', REGIMES)
def test_integer_model_does_not_depend_on_the_row_order(regime):
    B, V, fh, fw, tps, rows, wts, key = make_case('B3 V3 empty segment between live ones', regime)
    upmax = float(np.abs(rows).max())
    v0, q0, c0 = model_fixed(rows, wts, key, B * V, fh, fw, upmax)
    r2, w2, k2 = shuffle_inside_pairs(np.random.default_rng(1), rows, wts, key)
    v1, q1, c1 = model_fixed(r2, w2, k2, B * V, fh, fw, upmax)
    assert np.array_equal(q0, q1) and np.array_equal(v0.view(np.uint32), v1.view(np.uint32)) and not c0 and not c1
    assert np.abs(q0).max() > 0
    f64 = model_float64(rows, wts, key, B * V, fh, fw)
    quantum = 2.0 ** (fx_exponent(upmax) - 28)
    assert (np.abs(v0 - f64[0]) <= (f64[1] * 0.5 + 1) * quantum + np.abs(f64[0]) * 2.0 ** -23 + f64[2] * 2.0 ** -23).all()
    assert fx_exponent(1.0) == 1 and fx_exponent(0.75) == 0 and fx_exponent(0.0) == 0 and fx_exponent(np.inf) == 0 and fx_exponent(1e-38) == -90
    # a contribution beyond 2^42 quanta is clamped and told
    rows[0, 0], wts[0], key[0] = 40000.0, (1, 0, 0, 0), 4
    v2, q2, c2 = model_fixed(rows, wts, key, B * V, fh, fw, 1.0)
    assert c2 and abs(int(q2[0, 4, CHANNEL[0]])) >= 2 ** 42 - 2 ** 36


# ---- GPU part A: the stage alone against the models -------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hot(weights_np):
    from graspnerf_amd import weights
    from graspnerf_amd.hotpath import HotPath
    return HotPath(weights.pack_state_dict(weights_np, 'coarse'), weights.pack_state_dict(weights_np, 'fine'))


def _run(hot, case, fixed, path, upmax=0.0, neutralised_keys=0):
    import torch
    B, V, fh, fw, tps, rows, wts, key = case
    dray, dimg, raw, status, neutralised = hot.debug_feature_scatter(B, V, fh, fw, tps, torch.from_numpy(rows), torch.from_numpy(wts),
                                                                     torch.from_numpy(key), upmax=upmax, fixed=fixed, path=path)
    assert neutralised == neutralised_keys                    # 0: no input of the model tests holds a key outside its row's scene-view
    return dray.cpu().numpy(), dimg.cpu().numpy(), raw.cpu().numpy(), status


def _check_float(got, case, what):
    """|got - ref64| <= (2 n + 2) 2^-24 S per entry: the running fmaf sum of a piece rounds once per contribution (each time by at most
    2^-24 of a partial sum of absolute value <= S), the atomic adds of the (bin, chunk) pieces round at most once per piece, of which
    there are at most n, the unpack rounds nothing; + 2 for the second-order terms.  n = 0: exactly 0."""
    B, V, fh, fw, tps, rows, wts, key = case
    dray, dimg, raw, status = got
    ref, n, S = model_float64(rows, wts, key, B * V, fh, fw)
    r_ray, r_img = to_nchw(raw, B, V, fh, fw)
    assert np.array_equal(dray, r_ray) and np.array_equal(dimg, r_img), f'{what}: k_unpack_feat_grad changed a value'
    err, bound = np.abs(raw.astype(np.float64) - ref), (2 * n + 2) * 2.0 ** -24 * S
    worst = np.unravel_index(np.argmax(np.where(n > 0, err / np.where(bound > 0, bound, 1.0), 0.0)), err.shape)
    print(f'{what}: worst entry {tuple(int(i) for i in worst)}: err {err[worst]:.3e}, bound {bound[worst]:.3e}, n = {n[worst]}')
    assert (raw[n == 0] == 0).all(), f'{what}: an entry nothing was added to is not 0'
    assert (err <= bound).all(), f'{what}: entry {worst}: |got - ref| = {err[worst]:.3e} > {bound[worst]:.3e} (n = {n[worst]}, S = {S[worst]:.3e})'
    assert status == 0


@pytest.mark.gpu
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('name', CASES)
def test_scatter_stage_against_the_models(name, regime, hot):
    case = make_case(name, regime)
    B, V, fh, fw, tps, rows, wts, key = case
    for path, pname in ((1, 'LDS placement'), (2, 'scan + fill')):
        _check_float(_run(hot, case, False, path), case, f'{name} / {regime} / float / {pname}')
    upmax = float(np.abs(rows).max())
    want, want_q, clamped = model_fixed(rows, wts, key, B * V, fh, fw, upmax)
    assert not clamped
    shuffled = shuffle_inside_pairs(np.random.default_rng(7), rows, wts, key)
    runs = [_run(hot, case, True, 1, upmax), _run(hot, case, True, 2, upmax),
            _run(hot, (B, V, fh, fw, tps) + shuffled, True, 1, upmax), _run(hot, (B, V, fh, fw, tps) + shuffled, True, 2, upmax)]
    w_ray, w_img = to_nchw(want, B, V, fh, fw)
    for (dray, dimg, raw, status), what in zip(runs, ('LDS placement', 'scan + fill', 'shuffled rows, LDS placement', 'shuffled rows, scan + fill')):
        assert status == 0, what
        assert np.array_equal(raw, want_q), (name, regime, what, 'integer sums')
        assert np.array_equal(dray.view(np.uint32), w_ray.view(np.uint32)) and np.array_equal(dimg.view(np.uint32), w_img.view(np.uint32)), (name, regime, what)


@pytest.mark.gpu
def test_far_taps_of_the_last_column_and_row_are_skipped_whatever_they_weigh(hot):
    """Beyond the view kernel's promise (it parks zero far weights there): rows in the last column / row with non-zero far weights.
    The stage skips those taps (scatter_flush) and must not hand them on to the next bin either -- (y, fw - 1) and (y + 1, 0) are
    consecutive keys: this is what the `% fw` term of the carry condition is for."""
    rng = np.random.default_rng(11)
    B, V, fh, fw, pix = case_pixels('line end 40x30', rng)
    rows, wts, key = make_rows(rng, pix, fh, fw, 'normal')
    wts[:] = rng.uniform(0.1, 0.9, wts.shape).astype(np.float32)
    case = (B, V, fh, fw, pix.shape[2] // 16, rows, wts, key)
    for path in (1, 2):
        _check_float(_run(hot, case, False, path), case, f'non-zero far weights / path {path}')
        want, want_q, _ = model_fixed(rows, wts, key, B * V, fh, fw, 4.0)
        assert np.array_equal(_run(hot, case, True, path, 4.0)[2], want_q)


@pytest.mark.gpu
def test_a_contribution_beyond_the_fixed_point_range_is_clamped_and_told(hot):
    B, V, fh, fw, tps, rows, wts, key = make_case('cap80 dead rows interleaved', 'normal')
    # rows 1 and 4 belong to (tile 0, view 0): keys of scene-view 0.  4e4 x 2^27 quanta at upmax = 1 (e = 1) is beyond 2^42
    rows[1, 5], wts[1], key[1] = 40000.0, (1, 0, 0, 0), 4
    rows[4, 9], wts[4], key[4] = -70000.0, (0.5, 0.5, 0, 0), 3
    want, want_q, clamped = model_fixed(rows, wts, key, B * V, fh, fw, 1.0)
    assert clamped
    for path in (1, 2):
        dray, dimg, raw, status = _run(hot, (B, V, fh, fw, tps, rows, wts, key), True, path, 1.0)
        assert status & 8 == 8
        assert np.array_equal(raw, want_q)
        assert np.array_equal(dray.view(np.uint32), to_nchw(want, B, V, fh, fw)[0].view(np.uint32))


@pytest.mark.gpu
def test_debug_entry_takes_a_key_of_another_scene_view_as_a_dead_row(hot):
    """The one promise of the entry about wrong input: a key outside its own row's scene-view range is -1 before anything consumes it,
    and counted.  Keys that stay inside every buffer even unsanitised: -2, and a pixel of the neighbouring scene-view (two views of
    3 x 3 pixels: keys 0 .. 8 belong to view 0's rows, 9 .. 17 to view 1's)."""
    B, V, fh, fw, tps, rows, wts, key = make_case('cap80 dead rows interleaved', 'normal')
    view = (np.arange(key.size) // 16) % V
    live = np.nonzero(key >= 0)[0]
    wrong = live[::5]
    bad, dead = key.copy(), key.copy()
    bad[wrong] = np.where(np.arange(wrong.size) % 2 == 0, -2, key[wrong] + np.where(view[wrong] == 0, 9, -9))
    dead[wrong] = -1
    assert wrong.size >= 8 and (bad[wrong][1::2] >= 0).all() and (bad[wrong][1::2] < 18).all()
    for path in (1, 2):
        got = _run(hot, (B, V, fh, fw, tps, rows, wts, bad), False, path, neutralised_keys=wrong.size)
        _check_float(got, (B, V, fh, fw, tps, rows, wts, dead), f'wrong keys / path {path}')
        want, want_q, _ = model_fixed(rows, wts, dead, B * V, fh, fw, 4.0)
        assert np.array_equal(_run(hot, (B, V, fh, fw, tps, rows, wts, bad), True, path, 4.0, neutralised_keys=wrong.size)[2], want_q)


@pytest.mark.gpu
def test_debug_entry_refuses_what_it_cannot_run(hot):
    import torch
    from graspnerf_amd import _lib
    z = lambda *s: torch.zeros(*s)
    k = torch.full((32,), -1, dtype=torch.int32)
    with pytest.raises(_lib.GnrError):
        hot.debug_feature_scatter(1, 2, 3, 3, 1, z(32, 64), z(32, 4), k, path=3)
    with pytest.raises(_lib.GnrError):
        hot.debug_feature_scatter(1, 2, 200, 200, 1, z(32, 64), z(32, 4), k, path=1)      # 40 000 pixels do not fit the LDS placement
    with pytest.raises(_lib.GnrError):
        hot.debug_feature_scatter(1, 2, 0, 3, 1, z(32, 64), z(32, 4), k)
    dray, dimg, raw, status, neutralised = hot.debug_feature_scatter(1, 2, 3, 3, 1, z(32, 64), z(32, 4), k)
    assert float(dray.abs().max()) == 0 and float(dimg.abs().max()) == 0 and status == 0 and neutralised == 0


# ---- GPU parts B and C: whole backwards -------------------------------------------------------------------------------------------
RES, RN, DN = 4, 4, 4
CFG = {'depth_sample_num': DN, 'fine_depth_sample_num': DN, 'ray_mask_view_num': 2, 'ray_mask_point_num': 8}


def _hot_bwd(wnp):
    import torch
    from graspnerf_amd import weights
    from graspnerf_amd.hotpath import HotPath
    hp = HotPath(weights.pack_state_dict(wnp, 'coarse'), weights.pack_state_dict(wnp, 'fine'))
    can = {lvl: weights.canonical_blob(wnp, lvl) for lvl in ('coarse', 'fine')}
    hp.set_bwd_weights(weights.pack_bwd(can['coarse']), weights.pack_bwd(can['fine']))
    hp.can_dev = {lvl: torch.from_numpy(can[lvl]).cuda() for lvl in can}
    return hp


def _scene(W, H=640, seed=0):
    """One scene of two views H x W (feature maps H/4 x W/4), RN rays; the workspace box fills most of the image."""
    from graspnerf_amd.synth import make_scene
    f = 700.0 * H / 640
    return make_scene(seed, dict(V=2, H=H, W=W, rn=RN, K=[[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1]]), with_query_image=False)


def _upstream(seed=3):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, 1, RES, RES, RES, generator=g).cuda(), torch.randn(1, RN * DN, 65, generator=g).cuda(),
            torch.randn(1, RN * DN, 3, generator=g).cuda())


def _step(hp, ref, que, up, between=None):
    """Training forward + backward of the volume and of the coarse render pass -> (the six gradients, status, geo, sections).
    between(hp, scene, tws, n, dn): called after each training forward, before its backward."""
    import torch
    from graspnerf_amd.hotpath import batch_scenes
    bref, bque = batch_scenes([(ref, que)])
    bref = {k: torch.from_numpy(v).cuda() for k, v in bref.items()}
    bq = {k: torch.from_numpy(v).cuda() for k, v in bque.items() if k != 'imgs'}
    dvol, ds, dc = up
    prep = hp.prepare(bref, RES, RN, DN)
    hp.sample_volume_train(bref, RES, prepared=prep)
    scene, _, _, _, tws_v = hp._train_ctx                     # (scene, keep, ws, res, tws), as sample_volume_bwd unpacks it
    if between:
        between(hp, scene, tws_v, RES, 0)
    vol_g = hp.sample_volume_bwd(dvol, hp.can_dev['coarse'])
    _, _, geo, ctx = hp.render_chain_train(bq, None, 'coarse', CFG, prep)
    tws_r = ctx[3]                                            # (scene, keep, ws, tws, ...), as render_chain_bwd unpacks it
    if between:
        between(hp, scene, tws_r, RN, DN)
    ren_g = hp.render_chain_bwd(ctx, ds, dc)
    torch.cuda.synchronize()
    names = ['volume d_canonical', 'volume d_ray_feats', 'volume d_img_feats', 'render d_canonical', 'render d_ray_feats', 'render d_img_feats']
    sections = {'volume': hp.scatter_ws_sections(scene, tws_v, RES, 0), 'render': hp.scatter_ws_sections(scene, tws_r, RN, DN)}
    return dict(zip(names, [t.clone() for t in vol_g] + [t.clone() for t in ren_g])), hp.range_status(prep), geo, sections


def _autograd64(wnp, ref, que, depth, up):
    """float64 autograd over tests/reference_autograd.py on the CPU -> the four feature-map gradients."""
    import torch
    import reference_autograd as ag
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        d = lambda a: torch.from_numpy(np.asarray(a)).double()
        P = {k: d(v) for k, v in wnp.items()}
        dvol, ds, dc = (t.cpu().double() for t in up)
        out = []
        tref = {k: d(v) for k, v in ref.items()}
        tref['ray_feats'].requires_grad_(True); tref['img_feats'].requires_grad_(True)
        (ag.sample_volume(P, tref, RES) * dvol).sum().backward()
        out += [tref['ray_feats'].grad.clone(), tref['img_feats'].grad.clone()]
        tref['ray_feats'].grad = None; tref['img_feats'].grad = None
        q1 = {k: d(que[k]) for k in ('coords', 'pose', 'K', 'depth_range')}
        depth = depth.cpu().double()
        pts, qdir = ag.ray_points(q1, depth)
        h, w = ref['imgs'].shape[-2:]
        uv, z, mask, dirv = ag.project(pts, tref['poses'], tref['Ks'], h, w)
        f_ray, rgb, f_img = ag._gather(tref, uv, mask)
        near, far = -1 / q1['depth_range'][0], -1 / q1['depth_range'][1]
        di = (-1 / depth - near) / (far - near)
        half = torch.cat([di[:, 1:] - di[:, :-1], torch.full_like(di[:, :1], 1e6)], -1) / 2
        ext = torch.cat([half[:, :1], half], -1)
        hit, vis = ag.decode_hit_vis(P, 'dist_decoder.', f_ray, z, mask, tref['depth_range'], ext[:, :-1].reshape(-1), ext[:, 1:].reshape(-1))
        taps = {}
        qd = qdir[:, None].expand(RN, DN, 3).reshape(-1, 3)
        _, _, col = ag.aggregate(P, 'agg_net.', f_ray, rgb, f_img, hit, vis, mask, dirv, qd, pts, RN, DN, False, True, taps)
        v2 = taps['v2']
        wbar = (v2 / (v2.sum(0, keepdim=True) + 1e-8)).mean(0)
        stats = torch.cat([taps['mean'], taps['var'], wbar], -1)
        ((stats * ds[0]).sum() + (col.reshape(-1, 3) * dc[0]).sum()).backward()
        out += [tref['ray_feats'].grad, tref['img_feats'].grad]
        return out
    finally:
        torch.set_default_dtype(prev)


FEATS = ['volume d_ray_feats', 'volume d_img_feats', 'render d_ray_feats', 'render d_img_feats']


@pytest.mark.gpu
@pytest.mark.parametrize('W,placed,not_placed', [(960, 'k_scatter_place@', 'k_scatter_fill@'), (964, 'k_scatter_fill@', 'k_scatter_place@')])
def test_both_sides_of_the_placement_threshold(W, placed, not_placed, weights_np):
    """Feature maps of 160 x 240 = 38 400 pixels (the last size whose pixel counters fit the LDS: k_scatter_place) and of 160 x 241
    (the first on k_scatter_scan + k_scatter_fill), through sample_volume_bwd and a coarse render_chain_bwd."""
    import torch
    from graspnerf_amd import _lib
    from test_bwd_twins import _close
    from test_determinism import _feat_close
    ref, que = _scene(W)
    up = _upstream()
    hp = _hot_bwd(weights_np)
    _lib.timing_begin()
    try:
        flt, status, geo, sec = _step(hp, ref, que, up)
    finally:
        labels = _lib.timing_end()
    assert any(k.startswith(placed) for k in labels) and not any(k.startswith(not_placed) for k in labels), sorted(labels)
    assert ('k_scatter_scan@gnr_render_chain_bwd' in labels) == (W == 964)
    assert status == 0
    for leg in ('volume', 'render'):
        key = sec[leg]['key']
        assert int((key >= 0).sum()) * 2 >= key.numel(), (leg, int((key >= 0).sum()), key.numel())
    # fixed-point mode: the binned scatter is the direct scatter, bit for bit
    hp.feature_grad_mode(True)
    fixed, status, _, _ = _step(hp, ref, que, up)
    assert status & 8 == 0 and status == 0
    hp.set_option('direct_scatter', True)
    direct, status, _, _ = _step(hp, ref, que, up)
    hp.set_option('direct_scatter', False)
    assert status & 8 == 0
    for k in FEATS:
        assert float(fixed[k].abs().max()) > 0, k
        assert torch.equal(fixed[k], direct[k]), (k, float((fixed[k] - direct[k]).abs().max()))
        _feat_close(flt[k], fixed[k])
    want = _autograd64(weights_np, ref, que, geo['depth'][0], up)
    for k, r in zip(FEATS, want):
        _close(flt[k][0], r, k, rel=1e-3)
        _close(fixed[k][0], r, k + ' (fixed point)', rel=1e-3)


def _regime(name, wnp, ref):
    w = dict(wnp)
    if name == 'features x3000':
        return w, dict(ref, ray_feats=ref['ray_feats'] * np.float32(3000), img_feats=ref['img_feats'] * np.float32(3000)), 2
    k = 'dist_decoder.mean_decoder.0.weight'                 # 'a weight without an fp16 pair'
    w[k] = w[k].copy()
    w[k][3, 5] = 1e5
    return w, ref, 4


SENTINEL = 0x5a5a5a5a


def _poison_scatter(hp, scene, tws, n, dn):
    """On the stream of the forward that just ran: valid keys (a random pixel of each row's own scene-view), rows / wts = 0x71 bytes
    (1.19e30), list / cursor / nseg = a sentinel."""
    import torch
    s = hp.scatter_ws_sections(scene, tws, n, dn)
    N, V, npix = s['key'].numel(), scene.V, scene.fh * scene.fw
    tps = N // (scene.B * V * 16)
    i = torch.arange(N, device=s['key'].device)
    seg = (i // (16 * V * tps)) * V + (i // 16) % V
    g = torch.Generator().manual_seed(N)
    s['key'].copy_((seg * npix + torch.randint(0, npix, (N,), generator=g).to(seg.device)).to(torch.int32))
    for name in ('rows', 'wts'):
        s[name].view(torch.uint8).fill_(0x71)
    for name in ('list', 'cursor', 'nseg'):
        s[name].fill_(SENTINEL)


@pytest.mark.gpu
@pytest.mark.parametrize('W,H', [(128, 96), (964, 640)], ids=['24x32 LDS placement', '160x241 scan + fill'])
@pytest.mark.parametrize('regime', ['features x3000', 'a weight without an fp16 pair'])
def test_a_flagged_pass_consumes_nothing_it_did_not_write(regime, W, H, weights_np):
    """A range-flagged backward: k_view1_bwd_pw returns at its guard and parks no key, no weight, no row; its fp32 twin scatters
    directly.  With the scatter region of the training workspace holding valid-looking keys, huge rows and weights and a sentinel in
    list / cursor / nseg, the gradients are bitwise those of an unpoisoned GNR_OPT_FP32_CHAIN run, and `list` still holds the sentinel:
    nothing was placed, so nothing stale can be gathered."""
    import torch
    w, ref, want = _regime(regime, weights_np, _scene(W, H)[0])
    que = _scene(W, H)[1]
    up = tuple(t * s for t, s in zip(_upstream(), (1e-3, 1e-2, 1e-2)))
    hp = _hot_bwd(w)
    hp.feature_grad_mode(True)
    got, flags, _, sec = _step(hp, ref, que, up, between=_poison_scatter)
    assert flags & want == want, (regime, flags)
    clean = _hot_bwd(w)
    clean.feature_grad_mode(True)
    clean.force_fp32_chain(True)
    f32, _, _, _ = _step(clean, ref, que, up)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
        assert torch.equal(v, f32[k]), (regime, k, float((v - f32[k]).abs().max()), float(f32[k].abs().max()))
    for leg in ('volume', 'render'):
        assert bool((sec[leg]['list'] == SENTINEL).all()), f'{leg}: the scatter kernels placed rows of a pass whose view kernel parked none'
