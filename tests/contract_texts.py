"""What the tests/test_gpu_*contract_texts.py files share: libocc4d.so and the g++ twin loaded in one process -- the twin as a
second plain handle, never enabled --, zeros tensors that stay alive where each of them reads, and the parametrised test that hands
both the same rejected calls.  A file keeps its call builders, its REJECTED table and its accepted edges, and binds `libraries`
and the test rejected_test() returns in its own namespace, where pytest collects them."""
import ctypes

import numpy as np
import pytest
import torch

import occlusions4d_amd as pk

DEV = torch.device('cuda:0')


def p(t):
    return ctypes.c_void_p(t.data_ptr())


class HostPointer(ctypes.c_void_p):
    """A void pointer that keeps the numpy array it points into alive."""


def host_int32(*rows, width):
    """The pointer to a (len(rows), width) int32 array in host memory, for both libraries."""
    a = np.array(rows, np.int32).reshape(-1, width)
    pointer = HostPointer(a.ctypes.data)
    pointer.array = a
    return pointer


class zeros_on:
    """z(*shape, dtype): a zeros tensor on the device that stays alive as long as z does -- a call's pointers are real memory."""

    def __init__(self, device):
        self.device, self.alive = device, []

    def __call__(self, *shape, dtype=torch.int32):
        self.alive.append(torch.zeros(*shape, dtype=dtype, device=self.device))
        return self.alive[-1]


class float_zeros_on(zeros_on):
    """zeros_on for the headers whose operands are mostly fields: float32 unless the call says otherwise."""

    def __call__(self, *shape, dtype=torch.float32):
        return super().__call__(*shape, dtype=dtype)


@pytest.fixture(scope='module')
def libraries():
    hip = pk._lib.lib()
    twin = pk._lib.bind(ctypes.CDLL(pk.cpu_twin.build()), missing=lambda name: None)      # a second handle: enable() is not called
    assert not pk.cpu_twin.enabled() and hip.occ4d_is_cpu_twin() == 0 and twin.occ4d_is_cpu_twin() == 1
    return hip, twin


def rejected_test(REJECTED, zeros=zeros_on):
    """The test of a file's REJECTED table, rows (message fragment, call(L, z)): both libraries return EINVAL with the same
    occ4d_last_error() bytes, which hold the fragment.  `zeros`: the class of z (the file's default dtype)."""
    @pytest.mark.parametrize('fragment,call', REJECTED, ids=['%02d' % i for i in range(len(REJECTED))])
    def test_both_libraries_reject_with_the_same_text(libraries, fragment, call):
        hip, twin = libraries
        on_device, on_host = zeros(DEV), zeros('cpu')
        rc_hip = call(hip, on_device)
        text_hip = bytes(hip.occ4d_last_error())
        rc_twin = call(twin, on_host)
        text_twin = bytes(twin.occ4d_last_error())
        assert rc_hip == rc_twin == pk._lib.EINVAL
        assert text_hip == text_twin and fragment.encode() in text_hip, (text_hip, text_twin)
    return test_both_libraries_reject_with_the_same_text
