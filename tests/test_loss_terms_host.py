"""Host: the per-term loss values of training.implicit_loss (return_terms=True) on its torch path against the `terms` the
reference's own loss code recorded in the G14 fixtures (unweighted, order colour / density / segmentation / tracking), and
the layout rule that decides which calls the fused kernel takes.  The kernel itself: tests/test_gpu_loss_terms.py."""
import numpy as np
import pytest
import torch

import golden_cases as gc
from conftest import load_golden
import occlusions4d_amd as pk

CASES = gc.LOSS_CASES + gc.LOSS_COLOR_CASES


@pytest.mark.parametrize('static_shapes', [False, True], ids=['eager', 'static'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_terms_match_the_reference_fixtures(case, static_shapes):
    """Each of the four terms within 2e-6 of the fixture (the G14 gate of the total), a (4,) detached tensor; the total and
    its gradient are what return_terms=False gives."""
    g = load_golden('g14_loss_' + case['name'])
    raw_np, target_np = gc.loss_inputs(case)
    raw = torch.from_numpy(raw_np).requires_grad_(True)
    total, terms = pk.training.implicit_loss(raw, torch.from_numpy(target_np), static_shapes=static_shapes, return_terms=True,
                                             **gc.loss_kwargs(case))
    assert terms.shape == (4,) and terms.dtype == torch.float32 and not terms.requires_grad
    for k in range(4):
        print(case['name'], k, float(terms[k]), float(g['terms'][k]))
        assert abs(float(terms[k]) - float(g['terms'][k])) < 2e-6
    total.backward()
    raw2 = torch.from_numpy(raw_np).requires_grad_(True)
    plain = pk.training.implicit_loss(raw2, torch.from_numpy(target_np), static_shapes=static_shapes, **gc.loss_kwargs(case))
    assert torch.is_tensor(plain) and plain.shape == ()
    plain.backward()
    assert plain.item() == total.item() and torch.equal(raw.grad, raw2.grad)
    assert abs(plain.item() - float(g["total"][0])) < 2e-6
    weights = [case[k] for k in ('color_lw', 'density_lw', 'segmentation_lw', 'tracking_lw')]
    assert abs(sum(w * float(t) for w, t in zip(weights, terms)) - float(total)) < 2e-6


def test_terms_of_unweighted_terms_are_zero():
    raw_np, target_np = gc.loss_inputs(CASES[0])
    _, terms = pk.training.implicit_loss(torch.from_numpy(raw_np), torch.from_numpy(target_np), density_lw=0.0, color_lw=0.0,
                                         tracking_lw=0.5, color_mode='rgb_nosigmoid', return_terms=True)
    assert terms[0] == 0 and terms[1] == 0 and terms[2] == 0 and terms[3] > 0


@pytest.mark.parametrize('g,mode,classes,weights,ok', [
    (5, 'rgb_nosigmoid', 13, (1.0, 1.0, 0.0, 1.0), True),     # the published GREATER command: default classes, no such term
    (5, 'rgb', 13, (1.0, 0.0, 0.0, 0.0), True),               # density alone on a G = 5 decoder
    (18, 'rgb', 13, (1.0, 0.0, 0.6, 0.0), True),              # the published CARLA command
    (18, 'rgb_nosigmoid', 13, (0.7, 0.9, 0.6, 0.3), True),
    (29, 'hsv', 13, (0.7, 0.9, 0.6, 0.3), True),
    (24, 'bins', 13, (0.7, 0.9, 0.6, 0.3), True),
    (5, 'hsv', 13, (1.0, 1.0, 0.0, 0.0), False),              # no room for the hsv channels
    (4, 'rgb', 13, (1.0, 0.0, 0.0, 1.0), False),              # no tracking channel
    (16, 'hsv', 13, (1.0, 1.0, 0.6, 1.0), False),             # classes would overlap the colour channels
    (13, 'rgb', 13, (1.0, 0.0, 0.6, 0.0), False),             # classes would overlap the density logit
    (18, 'rgb', 13, (1.0, -1.0, 0.6, 0.0), False),
])
def test_fused_layout_rule(g, mode, classes, weights, ok):
    d, c, s, t = weights
    assert pk.training._fused_loss_layout(g, mode, classes, d, c, s, t) is ok
