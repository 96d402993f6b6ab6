"""The grid products of perform_inference together (products.py: surface, views, components, tracker, clearance, route in one call,
and through evaluate_clip) through the g++ twin, without a GPU: tests/products_cases.py, everything EQUAL, no tolerance.
tests/test_gpu_products.py runs the same comparisons on the device."""
import pytest
import torch

import products_cases as pc
import refine_cases as rc
import occlusions4d_amd as pk

CPU = torch.device('cpu')


@pytest.fixture
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


@pytest.fixture(scope='module')
def shared():
    pk.cpu_twin.enable()
    try:
        return rc.Shared(CPU)
    finally:
        pk.cpu_twin.disable()


def test_all_products_in_one_call(twin, shared):
    pc.check_all_at_once(shared)


def test_evaluate_clip_with_all_products(twin, shared):
    pc.check_clip_all_at_once(shared)


def test_first_error_in_the_order_of_validation_wins(twin, shared):
    pc.check_first_error_wins(shared)
