"""Shared by tests/test_products_host.py (g++ twin) and tests/test_gpu_products.py (HIP): all six grid products of perform_inference
(products.GridProduct: surface, views, components, tracker, clearance, route) in ONE call, against the calls that pass one of them
with the product it needs.  Both sides run the same code on the same device, so everything is compared EQUAL: np.array_equal and the
same dtype, no tolerance.  The shape is rc.CASE: 768 input points, the 14 x 14 x 9 grid of 1764 queries."""
import numpy as np
import pytest

import geodesic_cases as geo
import raycast_cases as ray
import refine_cases as rc
import occlusions4d_amd as pk

# (the option's keyword, the options it needs, the result key its arrays come back under, evaluate_clip's list keyword)
TABLE = [('surface', (), 'surface', 'meshes'), ('views', (), 'views', 'images'), ('components', (), 'components', 'objects'),
         ('tracker', ('components',), 'components', 'objects'), ('clearance', (), 'clearance', 'clearances'),
         ('route', ('clearance',), 'route', 'routes')]
KEYS = ['surface', 'views', 'components', 'clearance', 'route']            # in the order perform_inference adds them
NAMES = dict(surface=['vertices', 'faces'], views=['depth', 'cell', 'features'], components=['labels', 'table', 'link'],
             clearance=['dist2', 'nearest', 'inside2'], route=['cost', 'status', 'parent', 'paths', 'path_len'])


def options(shared, points, *keywords):
    """The test's option objects, made anew for every call (a Tracker remembers the call before): {keyword: option} of all six, or of
    `keywords` alone.  points: geodesic_cases' (seeds, goals) of the fixture, worked out once by the caller."""
    seeds, goals = points
    every = dict(surface=pk.surface.Surface(), views=ray.fixture_views(shared, channels=(0, 4)), components=pk.components.Components(),
                 tracker=pk.components.Tracker(), clearance=pk.distance.Clearance(nearest=True, inside=True),
                 route=pk.geodesic.Route(seeds, goals, parent=True))
    return {k: every[k] for k in (keywords or every)}


def same_product(got, want, names=None):
    """Two product dicts: the same names in the same order (`want` may lack the `names` a later product adds), equal arrays."""
    assert [k for k in got if names is None or k in names] == list(want), (list(got), list(want))
    for k in want:
        assert isinstance(got[k], np.ndarray) and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def check_keys(got):
    assert [k for k in got if k in KEYS] == KEYS
    for key in KEYS:
        assert list(got[key]) == NAMES[key] and all(isinstance(a, np.ndarray) for a in got[key].values()), key


def check_all_at_once(shared):
    """One call with all six options, under one host wait: every product's dict is that of the call with that option (and what it
    needs) alone, the rest is the dense call's; the rest also in track_mode 'all'."""
    points = geo.fixture_points(shared)
    with pytest.MonkeyPatch.context() as monkeypatch:
        calls = rc.count_waits(monkeypatch)
        got = rc.infer(shared.device, shared.inputs, **options(shared, points))
        assert calls['wait'] == 1
    assert (got['views']['cell'] >= 0).any() and len(got['surface']['faces']) > 0 and len(got['components']['table']) > 0
    assert got['route']['status'][0] == 1 and (got['route']['path_len'] != 0).any()           # the fixture's condition: nothing is empty
    check_keys(got)
    for keyword, needs, key, _ in TABLE:
        alone = rc.infer(shared.device, shared.inputs, **options(shared, points, keyword, *needs))
        assert [k for k in alone if k in KEYS] == [k for k in KEYS if k in needs + (key,)], keyword
        same_product(got[key], alone[key], None if keyword != 'components' else ['labels', 'table'])
    rc.same_result({k: v for k, v in got.items() if k not in KEYS}, shared.dense)
    got = rc.infer(shared.device, shared.inputs, track_mode='all', **options(shared, points))
    check_keys(got)
    rc.same_result({k: v for k, v in got.items() if k not in KEYS}, shared.dense_all)


def check_first_error_wins(shared):
    """Several things wrong at once: the first one in the order of validation is raised, before any decode -- perform_inference:
    refine, surface, views, components, tracker, clearance, route; evaluate_clip: route, clearance, tracker, components, views,
    surface."""
    order = ['surface', 'views', 'components', 'tracker', 'clearance', 'route']
    for i, first in enumerate(order):
        with pytest.raises(ValueError, match='^%s must be a ' % first):
            rc.infer(shared.device, shared.inputs, **{k: 0.5 for k in order[i:]})
    with pytest.raises(ValueError, match='^refine must be a GridRefine'):
        rc.infer(shared.device, shared.inputs, refine=0.5, **{k: 0.5 for k in order})
    points = geo.fixture_points(shared)
    seeds = points[0]
    with pytest.raises(ValueError, match='^tracker needs components='):
        rc.infer(shared.device, shared.inputs, tracker=pk.components.Tracker(), route=pk.geodesic.Route(seeds), point_sample_mode='random')
    with pytest.raises(ValueError, match="^route needs point_sample_mode 'grid'"):
        rc.infer(shared.device, shared.inputs, route=pk.geodesic.Route(seeds), point_sample_mode='random')
    with pytest.raises(ValueError, match='^components with by_class=True needs predict_segmentation=True'):
        rc.infer(shared.device, shared.inputs, components=pk.components.Components(by_class=True), clearance=0.5)
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    order = ['route', 'clearance', 'tracker', 'components', 'views', 'surface']
    for i, first in enumerate(order):
        with pytest.raises(ValueError, match='^%s must be a ' % first):
            pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', **{k: 0.5 for k in order[i:]})
    given = options(shared, points)
    for keyword, name in (('route', 'routes'), ('clearance', 'clearances'), ('components', 'objects'), ('views', 'images'), ('surface', 'meshes')):
        with pytest.raises(ValueError, match=r'^evaluate_clip\(%s=\.\.\.\) needs %s=<a list>: one ' % (keyword, name)):
            pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', **given)
        given[name] = []


def check_clip_all_at_once(shared):
    """evaluate_clip over the two frames of check_clip with all six options and the five lists: two entries per list, each the
    entry of the clip run with that option (and what it needs) alone."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    points = geo.fixture_points(shared)

    def clip(given):
        lists = {name: [] for keyword, _, _, name in TABLE if keyword in given}
        pcl_all = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True, **given, **lists)
        return pcl_all, lists

    pcl_all, got = clip(options(shared, points))
    dense = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True)
    assert sorted(got) == ['clearances', 'images', 'meshes', 'objects', 'routes'] and len(pcl_all) == len(dense) == 2
    for t in range(2):
        for a, b in zip(pcl_all[t], dense[t]):
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    for name, key in zip(('meshes', 'images', 'objects', 'clearances', 'routes'), KEYS):
        assert len(got[name]) == 2 and all(list(entry) == NAMES[key] for entry in got[name]), name
    for keyword, needs, _, name in TABLE:
        alone = clip(options(shared, points, keyword, *needs))[1]
        assert len(alone[name]) == 2, keyword
        for mine, theirs in zip(got[name], alone[name]):
            same_product(mine, theirs, None if keyword != 'components' else ['labels', 'table'])
