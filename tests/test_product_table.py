"""The table of a plan's products (graspnerf_amd/planner_session.py: PRODUCTS), without a GPU: every row's keywords exist where the table
says, a key nobody takes is refused by name on both entry points before anything touches a device, and plan_real(session=...) refuses
a session built without a product it is asked for, and the other way round.  And the one comparison behind that refusal,
grasp_post.same_params."""
import inspect
import types

import numpy as np
import pytest

from graspnerf_amd import planner
from graspnerf_amd.grasp_post import GRASP_UTILS_PROCESS, same_params
from graspnerf_amd.planner_session import PRODUCTS, PlannerSession, product_params

FRAMES, CAMS, K = [np.zeros((8, 8, 3), np.uint8)] * 4, [np.eye(4)] * 4, np.eye(3)


def stand_in(net, **session_kw):
    """What plan_real reads of a PlannerSession built with these product keywords (and the real route's everything else)."""
    return types.SimpleNamespace(net=net, selector_params=dict(GRASP_UTILS_PROCESS, order='index', top_k=None), surface_normals=False,
                                 voxel_size=planner.REAL_VOXEL_SIZE, **product_params(session_kw))


def test_the_table_names_every_product_once_in_the_sessions_order():
    assert [t.plan_kw for t in PRODUCTS] == ['clearance', 'closure', None, 'mesh', 'volume_depth', 'view_colors']
    assert [t.attr for t in PRODUCTS] == ['hand_params', 'closure_params', 'surface_params', 'mesh_params', 'volume_depth_params',
                                          'view_color_params']
    assert [t.cls.out for t in PRODUCTS if t.cls is not None] == ['hand', 'closure', 'surface', 'mesh', 'volume_depth']
    assert {t.plan_kw: t.keep for t in PRODUCTS if t.keep} == {'clearance': 'collision_free', 'closure': 'held'}
    assert all(t.cls.columns == (t.keep is not None) for t in PRODUCTS if t.cls is not None)
    assert product_params({}) == dict.fromkeys(t.attr for t in PRODUCTS)


@pytest.mark.parametrize('t', PRODUCTS, ids=lambda t: t.session_kw)
def test_keywords_and_refusals_of(t):
    assert inspect.signature(PlannerSession.__init__).parameters[t.session_kw].default is None
    net, cloud = object(), dict(surface=dict(rg=(-0.2, 0.2)))
    refused = pytest.raises(ValueError, match='real_session')
    if t.plan_kw is None:                                    # the cloud: every plan_real has it, a session need not
        with refused:
            planner.plan_real(net, FRAMES, CAMS, K, session=stand_in(net))
        with refused:
            planner.plan_real(net, FRAMES, CAMS, K, session=stand_in(net, surface=dict(rg=(-0.1, 0.2))))
        with pytest.raises(TypeError, match='unknown surface parameters'):
            product_params(dict(surface={'bogus': 1}))
        return
    for fn in (planner.plan_real, planner.real_session):
        assert inspect.signature(fn).parameters[t.plan_kw].default is False, fn
    with pytest.raises(TypeError, match=f"unknown {t.plan_kw} parameters \\['bogus'\\]"):
        planner.plan_real(None, FRAMES, CAMS, K, **{t.plan_kw: {'bogus': 1}})
    with pytest.raises(TypeError, match=f"unknown {t.plan_kw} parameters \\['bogus'\\]"):
        planner.real_session(None, 4, (8, 8), (32, 32), **{t.plan_kw: {'bogus': 1}})
    with refused:                                            # built without it, asked for it
        planner.plan_real(net, FRAMES, CAMS, K, session=stand_in(net, **cloud), **{t.plan_kw: True})
    with refused:                                            # built with it, not asked for it
        planner.plan_real(net, FRAMES, CAMS, K, session=stand_in(net, **cloud, **{t.session_kw: {}}))
    if t.noun is not None:
        with pytest.raises(ValueError, match=f'built for another {t.noun} \\(build it with planner.real_session'):
            planner.plan_real(net, FRAMES, CAMS, K, session=stand_in(net, **cloud), **{t.plan_kw: True})


def test_refusals_come_in_order_parameters_views_session():
    net = object()
    with pytest.raises(TypeError, match='unknown closure parameters'):           # ... before the view count
        planner.plan_real(net, FRAMES[:3], CAMS[:3], K, closure={'bogus': 1}, session=stand_in(net))
    with pytest.raises(ValueError, match='at least 4 views'):                    # ... before the session
        planner.plan_real(net, FRAMES[:3], CAMS[:3], K, session=stand_in(net))


def test_same_params():
    assert same_params(None, None) and not same_params(None, {}) and not same_params({}, None)
    assert not same_params(None, dict(iso=0.0)) and not same_params(dict(iso=0.0), None)
    asked = dict(iso=0.25, step=0.5)
    assert same_params(asked, dict(asked)) and same_params(asked, dict(asked, origin=(0.0, 0.0, 0.0)))      # a further key of the session's
    assert not same_params(dict(asked, origin=(0.0, 0.0, 0.0)), asked)                                      # ... but none of the asker's
    assert not same_params(asked, dict(asked, iso=0.5))
    assert same_params(dict(asked, filter=True), asked) and same_params(dict(asked, filter=True), dict(asked, filter=False))
    ext = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    assert same_params(dict(extrinsics=ext, hw=(5, 7)), dict(extrinsics=ext.copy(), hw=(5, 7)))             # arrays by value
    assert not same_params(dict(extrinsics=ext), dict(extrinsics=ext + 1)) and not same_params(dict(extrinsics=ext), dict(extrinsics=ext[:1]))
    assert not same_params(dict(extrinsics=ext), dict(extrinsics=None)) and not same_params(dict(extrinsics=None), dict(extrinsics=ext))
    assert same_params(dict(extrinsics=None), dict(extrinsics=None))
    assert same_params(dict(rg=(-0.2, 0.2)), dict(rg=[-0.2, 0.2])) and same_params(dict(fill=(0.0, 0.0, 0.0)), dict(fill=(0, 0, 0)))
