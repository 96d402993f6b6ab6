"""GPU: the decoder's query prelude (include/ext/occ4d_prelude.h, inference.QueryPrelude).  The same kernels run on the same
operands whether the front end is launched once over all queries beside the encoder or once per mini-batch inside the
decode, and every row depends on its own query alone: so every comparison here is torch.equal, never a tolerance.

Shapes: model_args(kind, 1536), the smallest cloud the pruned sampler serves (levels 512 / 171 / 57: still >= 16 neighbours);
mini-batches of 2304 queries (one DECODE_ALIGN) over 2 * 2304 + 7 queries = three mini-batches with a 7-row tail, so both
decode streams are in use; 100 queries = one short mini-batch."""
import pytest
import torch

import occlusions4d_amd as pk
import query_prelude_cases as host

pytestmark = pytest.mark.gpu

BATCH = 2304
N_LONG = 2 * BATCH + 7


class Case:
    def __init__(self, kind):
        pa, ia, self.inf = pk.configs.model_args(kind, 1536)
        esd, dsd = pk.configs.synthetic_weights(pa, ia, 11)
        self.enc = pk.model.PointCompletionNetV3(**pa).cuda().eval()
        self.enc.load_state_dict(esd)
        self.dec = pk.implicit.LocalPclResnetFC(**ia).cuda().eval()
        self.dec.load_state_dict(dsd)
        self.pcl = pk.configs.synthetic_pcl(kind, 1536, 4, seed=11).cuda()
        (x0, x1), (y0, y1), (z0, z1) = pk.configs.input_cuboid(kind)
        g = torch.Generator().manual_seed(12)
        u = torch.rand((N_LONG, 3), generator=g)
        lo, hi = torch.tensor([x0, y0, z0]), torch.tensor([x1, y1, z1])
        self.queries = torch.cat([lo + u * (hi - lo), torch.randint(0, 4, (N_LONG, 1), generator=g).float()], dim=1).cuda()
        with torch.no_grad(), pk.kernels(query_prelude=False):
            self.ref = self.run(N_LONG)                   # computed once, shared, never written

    def run(self, n):
        out, _ = pk.distributed.sharded_inference(self.pcl, self.queries[:n], self.enc, self.dec, BATCH, self.inf['color_mode'],
                                                  self.inf['predict_segmentation'])
        torch.cuda.synchronize()
        return out


@pytest.fixture(scope='module', params=['greater', 'carla'])
def case(request):
    return Case(request.param)


@pytest.fixture
def calls(monkeypatch):
    """How often each of the two forward entries and the prelude ran."""
    count = dict(fwd=0, fwd_prelude=0, prelude=0)
    for key, name in (('fwd', 'decoder_query_fwd'), ('fwd_prelude', 'decoder_query_fwd_prelude'), ('prelude', 'decoder_query_prelude')):
        real = getattr(pk.ops, name)

        def counted(*a, _real=real, _key=key, **k):
            count[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(pk.ops, name, counted)
    return count


@pytest.mark.parametrize('n', [N_LONG, 100])
def test_switch_on_equals_switch_off(case, calls, n):
    with torch.no_grad(), pk.kernels(query_prelude=True):
        got = case.run(n)
    assert calls == dict(fwd=0, fwd_prelude=-(-n // BATCH), prelude=1)
    # (rows are independent and the squash is per element: the first n rows of the long run are the short run)
    assert torch.equal(got, case.ref[:n])
    buf = case.dec._prelude_buffers[case.queries.device]
    assert buf['n'] == n and buf['x0'] is not None and buf['m'] == pk.distributed.abstract_shape(case.enc, 1536)[0]


def test_switch_off_runs_the_old_entry_only(case, calls):
    with torch.no_grad(), pk.kernels(query_prelude=False):
        got = case.run(100)
    assert calls == dict(fwd=1, fwd_prelude=0, prelude=0) and torch.equal(got, case.ref[:100])


def test_lists_only_when_x0_is_over_the_cap(case, calls, monkeypatch):
    monkeypatch.setattr(pk.implicit, 'PRELUDE_X0_MAX', 0)
    with torch.no_grad(), pk.kernels(query_prelude=True):
        got = case.run(N_LONG)
    assert calls == dict(fwd=0, fwd_prelude=3, prelude=1)
    assert case.dec._prelude_buffers[case.queries.device]['x0'] is None
    assert torch.equal(got, case.ref)


def test_early_abstract_coordinates_are_the_encoders(case):
    with torch.no_grad():
        xyz, ev = case.enc.abstract_xyz_early(case.pcl)
        pcl_abstract, _, _ = case.enc(case.pcl, False)
    ev.synchronize()
    torch.cuda.synchronize()
    assert tuple(xyz.shape) == (pk.distributed.abstract_shape(case.enc, 1536)[0], 3)
    assert torch.equal(xyz, pcl_abstract[0, :, :3])


def test_prelude_rows_are_the_per_mini_batch_searches(case):
    """What occ4d_decoder_query_fwd_f32 launches for a mini-batch -- the Euclidean search with distances, the weights, the
    squared-distance search, the Fourier features and lin_in, each over the mini-batch's rows -- against the prelude's single
    launches over all rows."""
    with torch.no_grad():
        pcl_abstract, _, _ = case.enc(case.pcl, False)
        xyz = pk.ops.copy_rows(pcl_abstract[0, :, :3])
        buf = case.dec.query_prelude(case.queries, xyz)
        for b in range(0, N_LONG, BATCH):
            q = case.queries[b:b + BATCH]
            idx8, dist = pk.ops.knn(q, xyz, 8, metric=1, return_dist=True)
            assert torch.equal(buf['idx_local'][b:b + BATCH], idx8)
            assert torch.equal(buf['w_local'][b:b + BATCH], pk.ops.interp_weights(dist))
            assert torch.equal(buf['idx_cross'][b:b + BATCH], pk.ops.knn(q, xyz, 14, metric=0))
            pe = pk.ops.posenc(q, case.dec.pos_encoding_freqs, float(torch.tensor(0.1, dtype=torch.float32)))   # (the struct's fp32 base)
            assert torch.equal(buf['x0'][b:b + BATCH], pk.ops.linear(pe, case.dec.lin_in.weight, case.dec.lin_in.bias))


@pytest.mark.parametrize('precision', ['f32', 'bf16x6', 'f16x3'])
@pytest.mark.parametrize('with_x0', [True, False], ids=['x0', 'lists_only'])
def test_c_abi_forward_entries_agree(precision, with_x0):
    """300 rows (neither a multiple of 128 nor of 9) against m = 57, per selection: the entry on the prelude's rows = the entry
    that searches itself, outputs and penultimate activations."""
    dec, xyz, feats, fglobal, q = host.scene_of('greater', 'cuda')
    with torch.no_grad(), pk.kernels(precision=precision):
        (o_ref, p_ref), (o, p), _ = host.forward_both_ways(dec, xyz, feats, fglobal, q, with_x0)
    torch.cuda.synchronize()
    assert torch.isfinite(o_ref).all() and torch.equal(o, o_ref) and torch.equal(p, p_ref)


def test_hip_library_states_the_shared_contract():
    dec, xyz, feats, fglobal, q = host.scene_of('greater', 'cuda')
    w, _, _ = dec.path_weights()
    buf = host.prelude_buffers(w, host.ROWS, 'cuda', True)
    with pytest.raises(AssertionError, match='m = 7 abstract points cannot serve the 8 / 14 neighbours'):
        pk.ops.decoder_query_prelude(w, xyz[:7].contiguous(), q, buf['idx_local'], buf['w_local'], buf['idx_cross'], buf['x0'],
                                     buf['workspace'])


def test_second_identical_call_allocates_nothing(case):
    with torch.no_grad(), pk.kernels(query_prelude=True):
        case.run(N_LONG)
        case.run(N_LONG)
        buffers = case.dec._prelude_buffers[case.queries.device]
        ptrs = {k: v.data_ptr() for k, v in buffers.items() if torch.is_tensor(v)}
        streams = {k: [s.cuda_stream for s in v] for k, v in pk.inference._STREAMS.items()}
        reserved, segments = torch.cuda.memory_reserved(), torch.cuda.memory_stats()['segment.all.allocated']
        for _ in range(3):
            case.run(N_LONG)
    assert torch.cuda.memory_reserved() == reserved and torch.cuda.memory_stats()['segment.all.allocated'] == segments
    assert case.dec._prelude_buffers[case.queries.device] is buffers
    assert {k: v.data_ptr() for k, v in buffers.items() if torch.is_tensor(v)} == ptrs
    assert {k: [s.cuda_stream for s in v] for k, v in pk.inference._STREAMS.items()} == streams
