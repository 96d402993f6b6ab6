"""The instance statistics on the HIP path (csrc/inststats.hip): the case matrix and the InstanceStats checks of
tests/test_inst_host.py on the device (the kernels and the g++ twin share their per-row and per-id source, csrc/inst_math.hpp),
results that do not depend on the stream or the run, and perform_inference / evaluate_clip in track_mode 'all' with an
InstanceStats against the numpy restatement of tests/inst_cases.py.  Frame tables and counts EQUAL, sums within 1e-9 relative."""
import pytest
import torch

import inst_cases as ic
import occlusions4d_amd as pk

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def test_matrix_against_the_restatement():
    assert ic.check_matrix(DEV) == len(ic.matrix())


def test_rounding_ties_go_to_even():
    ic.check_ties_round_to_even(DEV)


def test_threshold_and_radius_are_compared_as_the_split_and_the_label_do():
    ic.check_thresholds(DEV)


def test_results_do_not_depend_on_the_stream_or_the_run():
    """A repeated call and three streams: equal bits (integer atomics are order-free, the double sums have one fixed order)."""
    torch.cuda.synchronize()
    ic.check_repeatable(DEV, streams=[torch.cuda.Stream() for _ in range(3)])
    torch.cuda.synchronize()


def test_a_frame_folded_twice_doubles_every_entry():
    ic.check_twice_doubles(DEV)


def test_summary_and_frame_tables_of_the_hand_made_frame():
    ic.check_hand_summary(DEV)


def test_merge_state_and_bad_groups():
    ic.check_merge_and_state(DEV)


def test_argument_errors():
    ic.check_argument_errors(DEV)


def test_host_tensors_are_rejected():
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        pk.ops.inst_fold(torch.zeros(ic.frame_len(2), dtype=torch.int64), torch.zeros(9, dtype=torch.int64), torch.zeros(4, dtype=torch.float64),
                         n_ids=2)


def test_track_mode_all_is_scored_end_to_end(monkeypatch):
    ic.check_end_to_end(DEV, monkeypatch)


def test_evaluate_clip_adds_every_frame():
    ic.check_clip_end_to_end(DEV)
