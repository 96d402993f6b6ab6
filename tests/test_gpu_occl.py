"""Per-instance visibility on the HIP path (csrc/idhist.hip): the case matrix and the reference's fixtures of
tests/test_occl_host.py on the device (the kernel and the g++ twin share their per-row source), tables that do not depend on the
stream or the run, the clip's device -> host reads, and the clip's ids through the point sampler.  Everything EQUAL."""
import numpy as np
import pytest
import torch

import gen_occl_fixture as gen
import occl_cases as oc
import occlusions4d_amd as pk

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.mark.parametrize('n', oc.ROW_COUNTS)
def test_histogram_case_matrix(n):
    assert oc.check_matrix(n, DEV) == 3 * 3 * (2 * 3 + 1)


def test_histogram_argument_errors():
    oc.check_argument_errors(DEV)


def test_tables_do_not_depend_on_the_stream_or_the_run():
    """Three streams at once and a repeated run: integer tables are order-free."""
    n, n_ids, S = 262401, 12, 48
    rng = np.random.default_rng(11)
    rows, key = oc.make_rows(n, n_ids, 'mixed', rng)
    off = oc.offsets_for(n, S, rng)
    want = oc.restate(rows, oc.COL, off, n_ids, key, oc.PRED_COL, (4.0, 10.0))
    r = torch.from_numpy(np.ascontiguousarray(rows.base)).to(DEV)[:, :oc.D]
    k, o = torch.from_numpy(key).to(DEV), torch.from_numpy(off).to(DEV)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    outs = []
    for _ in range(2):
        for st in streams:
            with torch.cuda.stream(st):
                outs.append(pk.ops.id_histogram(r, oc.COL, o, n_ids, key=k, pred_col=oc.PRED_COL, pred_values=(4.0, 10.0)))
    torch.cuda.synchronize()
    for out in outs:
        assert np.array_equal(out.cpu().numpy().astype(np.int64), want)


def test_bad_offsets_stay_inside_the_arrays():
    """The device cannot see the offsets on the host: whatever they hold, the counted rows are the n rows (every row lands
    in some segment's table) and nothing outside `counts` is written (the guard rows stay zero)."""
    n, n_ids = 1000, 12
    rows, _ = oc.make_rows(n, n_ids, 'mixed', np.random.default_rng(3))
    r = torch.from_numpy(np.ascontiguousarray(rows.base)).to(DEV)[:, :oc.D]
    guard = torch.zeros((5, n_ids + 2), dtype=torch.int32, device=DEV)
    for bad in ([0, 700, 300, 1000], [0, 100, 200, 400], [5, 5, 5, 5]):
        guard.zero_()
        pk.ops.id_histogram(r, oc.COL, torch.tensor(bad, dtype=torch.int64, device=DEV), n_ids, out=guard[1:4])
        assert int(guard[1:4].sum()) == n and int(guard[0].sum()) == 0 and int(guard[4].sum()) == 0


@pytest.mark.parametrize('name', oc.GOLDEN_NAMES)
def test_valo_ids_equal_the_reference(name):
    oc.check_valo_golden(name, DEV)
    oc.check_valo_golden(name, DEV, n_ids=1)                        # (the step-by-step path)


@pytest.mark.parametrize('name', [c[0] for c in gen.GREATER_CASES])
def test_choose_track_id_equals_the_reference(name):
    oc.check_track_golden(name, DEV)
    oc.check_track_golden(name, DEV, n_ids=1)


def test_valo_ids_reads_the_device_once():
    args, _ = oc.golden_arguments('carla_unfilt', DEV)
    with oc.TransferCount() as count:
        pk.occlusion.valo_ids(**args)
    assert count.n == 1


@pytest.mark.parametrize('name', [c[0] for c in gen.GREATER_CASES])
def test_greater_clip_with_and_without_the_new_arguments(name):
    got = oc.check_greater_clip(name, DEV)
    assert got[0].is_cuda
    if name == 'greater_unfilt':
        oc.through_the_sampler(got, 'greater', 'none', 5.0)


@pytest.mark.parametrize('name', [c[0] for c in gen.CARLA_CASES])
def test_carla_clip_with_and_without_the_new_arguments(name):
    got = oc.check_carla_clip(name, DEV)
    if name == 'carla_unfilt':
        oc.through_the_sampler(got, 'carla', 'ivalo', 16.0)


@pytest.mark.parametrize('name', ['greater_unfilt', 'greater_normal', 'carla_unfilt', 'carla_normal'])
def test_clip_makes_at_most_one_more_read(name):
    greater = name.startswith('greater')
    run = oc.greater_clip if greater else oc.carla_clip
    case = (gen.GREATER_BY_NAME if greater else gen.CARLA_BY_NAME)[name]
    with oc.TransferCount() as plain:
        run(name, DEV)
    extra = dict(live_occl_mode=case[2])
    if greater:
        extra['track_mode'] = case[3]
    with oc.TransferCount() as more:
        run(name, DEV, **extra)
    assert plain.n <= more.n <= plain.n + 1, (plain.n, more.n)
