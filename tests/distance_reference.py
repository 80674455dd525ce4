"""Statement of the distance field of a volume (include/gnr.h, gnr_volume_distance_fwd) -- TEST INFRASTRUCTURE ONLY, the arbiter of
csrc/gnr_distance.hip.  The squared distances are integers: scipy.ndimage.distance_transform_edt's feature transform gives a nearest
site per voxel and the squares of the index differences are summed as integers, never a float distance squared.  scipy's choice among
several nearest sites is its own, so the nearest site of the header -- the smallest linear index among those that attain the distance --
is stated by exhaustive search (R <= 12), and for larger volumes checked for what it must be: a site, in range, that attains d2.  `esdf`
is one correctly rounded float64 operation per line in the header's order, rounded once to float32.  Everything is compared with
np.array_equal."""
import numpy as np
from scipy import ndimage

f32, f64 = np.float32, np.float64
EXHAUSTIVE_MAX_R = 12


def solid(vol, level=0.0, lower=None, z_min=0):
    """[R,R,R] bool: lower < (double)v < level and k >= z_min; a NaN is not solid (objects_reference.solid's rule)."""
    v = np.asarray(vol, f32).astype(f64)
    with np.errstate(invalid='ignore'):
        s = (v < f64(level)) & ((-np.inf if lower is None else f64(lower)) < v)
    s[:, :, :int(z_min)] = False
    return s


def grid(R):
    """[3,R,R,R] int64: every voxel's own (i, j, k)."""
    return np.stack(np.meshgrid(*(np.arange(R, dtype=np.int64),) * 3, indexing='ij'))


def edt(sites):
    """sites [R,R,R] bool -> (d2 [R,R,R] int32, nearest [R,R,R] int32): the squared distance to the nearest site as an integer and A
    nearest site (scipy's choice among several);  without a site 3 R^2 and -1."""
    R = sites.shape[0]
    if not sites.any():
        return np.full(sites.shape, 3 * R * R, np.int32), np.full(sites.shape, -1, np.int32)
    at = ndimage.distance_transform_edt(~sites, return_distances=False, return_indices=True).astype(np.int64)
    d2 = ((at - grid(R)) ** 2).sum(0)
    return d2.astype(np.int32), ((at[0] * R + at[1]) * R + at[2]).astype(np.int32)


def exhaustive(sites):
    """The same by search over every (voxel, site) pair, R <= 12: d2, and the nearest site with the smallest linear index."""
    R = sites.shape[0]
    assert R <= EXHAUSTIVE_MAX_R
    if not sites.any():
        return np.full(sites.shape, 3 * R * R, np.int32), np.full(sites.shape, -1, np.int32)
    own = grid(R).reshape(3, -1).T                                             # [N,3], in linear order
    lin = np.flatnonzero(sites.ravel())                                        # ascending: argmin's first is the smallest index
    d = ((own[:, None, :] - own[lin][None, :, :]) ** 2).sum(-1)                # [N,S]
    return d.min(1).astype(np.int32).reshape(sites.shape), lin[d.argmin(1)].astype(np.int32).reshape(sites.shape)


def invalid_nearest(sites, d2, nearest):
    """[R,R,R] bool: where `nearest` is not what it must be -- in range, a site, at squared distance d2 (-1 everywhere without a site)."""
    R = sites.shape[0]
    if not sites.any():
        return nearest != -1
    ok = (nearest >= 0) & (nearest < R ** 3)
    at = np.stack(np.unravel_index(np.where(ok, nearest, 0), sites.shape)).astype(np.int64)
    return ~(ok & sites.ravel()[np.where(ok, nearest, 0)] & (((at - grid(R)) ** 2).sum(0) == d2))


def esdf(is_solid, d2_solid, d2_free, scale, surface_offset=0.5):
    """t = sqrt((double)d2);  t = t - surface_offset;  t = t * scale;  d2 = d2_solid at a free voxel, d2_free and -t at a solid one."""
    t = np.sqrt(np.where(is_solid, d2_free, d2_solid).astype(f64))
    t = t - f64(surface_offset)
    t = t * f64(scale)
    return np.where(is_solid, -t, t).astype(f32)


def nearest_label(labels, nearest_solid):
    """labels [R,R,R] int32 at nearest_solid; 0 where that is -1."""
    return np.where(nearest_solid >= 0, labels.ravel()[np.maximum(nearest_solid, 0)], 0).astype(np.int32)


def distance(vol, scale=1.0, level=0.0, lower=None, z_min=0, surface_offset=0.5, search=None):
    """vol [B,R,R,R] -> dict of solid [B,R,R,R] bool, d2_solid, d2_free int32, esdf float32, and -- with search (default: R <= 12) --
    nearest_solid, nearest_free int32 by exhaustive search."""
    vol = np.asarray(vol, f32)
    search = vol.shape[-1] <= EXHAUSTIVE_MAX_R if search is None else search
    out = {k: [] for k in ('solid', 'd2_solid', 'd2_free', 'esdf') + (('nearest_solid', 'nearest_free') if search else ())}
    for v in vol:
        s = solid(v, level, lower, z_min)
        (ds, ns), (df, nf) = (exhaustive(m) if search else edt(m) for m in (s, ~s))
        out['solid'].append(s)
        out['d2_solid'].append(ds)
        out['d2_free'].append(df)
        out['esdf'].append(esdf(s, ds, df, scale, surface_offset))
        if search:
            out['nearest_solid'].append(ns)
            out['nearest_free'].append(nf)
    return {k: np.stack(a) for k, a in out.items()}
