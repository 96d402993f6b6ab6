"""The running merge of the per-instance reruns on the HIP path (csrc/trackmerge.hip): the case matrix, the reference's fixtures
and the fused-versus-squash comparison of tests/test_track_host.py on the device (the kernels and the g++ twin share their
per-element source), results that do not depend on the stream or the run, and perform_inference / evaluate_clip in track_mode
'all' with the merge on the device against the merge on the host.  Everything EQUAL.

If the two modes ever differ end to end, compare the per-rerun raw outputs of the two calls first: the merge itself is pinned
by the matrix."""
import numpy as np
import pytest
import torch

import gen_track_fixture as gen
import track_cases as tc
import occlusions4d_amd as pk

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.mark.parametrize('name', gen.NAMES)
def test_merge_equals_the_reference(name):
    tc.check_golden(name, DEV)


@pytest.mark.parametrize('n', tc.ROW_COUNTS)
def test_merge_case_matrix(n):
    assert tc.check_matrix(n, DEV) == tc.cells_of(n)


def test_argument_errors():
    tc.check_argument_errors(DEV)


def test_merge_does_not_depend_on_the_stream_or_the_run():
    """Three streams at once and a repeated call: equal bits (no atomics, every element has one owner)."""
    n, g, K, track_col = 262401, 5, 5, 4
    rng = np.random.default_rng(17)
    raw = tc.raw_runs(n, g, K, rng)
    codes = [1, 1, 2, 0, 1]
    ids = [9, 2, 4095, 0, 5]
    runs = [torch.from_numpy(raw[k]).to(DEV) for k in range(K)]
    want = tc.restate(ids, [pk.ops.squash(r.clone(), codes).cpu().numpy() for r in runs], track_col)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    outs = []
    for _ in range(2):
        for st in streams:
            with torch.cuda.stream(st):
                outs.append(tc.merge_on(DEV, ids, runs, track_col, codes)[2])
    torch.cuda.synchronize()
    for out in outs:
        assert tc.same_bits(out.cpu().numpy(), want)


def test_device_merge_equals_host_merge_end_to_end(monkeypatch):
    """... and waits once, and never merges on the host."""
    res = tc.check_modes_agree(DEV, monkeypatch)
    assert res['device']['implicit_output'].shape[0] >= 1500 and res['device']['implicit_output'].shape[1] == 5


def test_clip_in_all_mode_reuses_one_encode_per_instance(monkeypatch):
    tc.check_clip_reuses_the_encodes(DEV, monkeypatch)
