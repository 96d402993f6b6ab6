"""The grid products of perform_inference together on the HIP path: the comparisons of tests/test_products_host.py on the device
(tests/products_cases.py), everything EQUAL, no tolerance."""
import pytest
import torch

import products_cases as pc
import refine_cases as rc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def shared():
    return rc.Shared(DEV)


def test_all_products_in_one_call(shared):
    pc.check_all_at_once(shared)


def test_evaluate_clip_with_all_products(shared):
    pc.check_clip_all_at_once(shared)


def test_first_error_in_the_order_of_validation_wins(shared):
    pc.check_first_error_wins(shared)
