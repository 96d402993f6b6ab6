"""Where the decode's query front end runs in a step, from a rocprofv3 --kernel-trace CSV of the bench command
(rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python bench.py --gpus 1 --steps 4 --warmup 2):
the front-end kernels' launches, time, first start and last end in the LAST complete step, against the start and end of the
encoder's sampling chain (the long fps_bucket_kernel launch), and that launch's duration over all steps of the trace.
Usage: python profiles/prelude_timeline.py <kernel_trace.csv> [label]"""
import csv
import sys

FRONT_END = [('knn_kernel<8, 1, int, 4>', 'search 8 (Euclidean, with distances)'), ('knn_kernel<16, 0, int, 4>', 'search 14 (squared distance)'),
             ('interp_weights_kernel', 'interpolation weights'), ('posenc_kernel', 'Fourier features'),
             ('linear_kernel<13, 1', 'lin_in (68 -> 416)')]


def short(name):
    return name.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    label = sys.argv[2] if len(sys.argv) > 2 else sys.argv[1]
    for r in rows:
        r['s'], r['e'], r['name'] = int(r['Start_Timestamp']), int(r['End_Timestamp']), short(r['Kernel_Name'])
    rows.sort(key=lambda r: r['s'])
    # a step ends with the squash of its outputs; the chain is the long fps_bucket_kernel launch of a step (the early
    # coordinates' launch of the same kernel is a ninth of it)
    fps = [r for r in rows if 'fps_bucket_kernel' in r['name']]
    assert fps, 'no fps_bucket_kernel in the trace'
    longest = max(r['e'] - r['s'] for r in fps)
    chains = [r for r in fps if r['e'] - r['s'] > longest / 2]
    early = [r for r in fps if r['e'] - r['s'] <= longest / 2]
    ends = [i for i, r in enumerate(rows) if 'squash_kernel' in r['name']]
    assert len(ends) >= 2, 'need at least two steps in the trace'
    seg = rows[ends[-2] + 1:ends[-1] + 1]
    t0 = seg[0]['s']
    chain = [r for r in seg if r in chains]
    assert len(chain) == 1, 'one sampling chain per step expected, found %d' % len(chain)
    c_s, c_e = (chain[0]['s'] - t0) / 1e3, (chain[0]['e'] - t0) / 1e3
    print('%s' % label)
    print('last step: %d kernels, %.3f ms from first start to last end' % (len(seg), (max(r['e'] for r in seg) - t0) / 1e6))
    print('sampling chain (%s): %9.1f .. %9.1f us  (%.1f us)' % (chain[0]['name'][:32], c_s, c_e, c_e - c_s))
    for r in seg:
        if r in early:
            print('early coordinates (same kernel): %9.1f .. %9.1f us  (%.1f us)' % ((r['s'] - t0) / 1e3, (r['e'] - t0) / 1e3,
                                                                                  (r['e'] - r['s']) / 1e3))
    print('%-38s %8s %10s %11s %11s %s' % ('front-end kernel', 'launches', 'time us', 'first start', 'last end', 'ended before the chain did'))
    total = 0.0
    for key, what in FRONT_END:
        ks = [r for r in seg if r['name'].startswith(key)]
        if not ks:
            print('%-38s %8d' % (what, 0))
            continue
        t = sum(r['e'] - r['s'] for r in ks) / 1e3
        total += t
        print('%-38s %8d %10.1f %11.1f %11.1f %d of %d' % (what, len(ks), t, (min(r['s'] for r in ks) - t0) / 1e3,
                                                          (max(r['e'] for r in ks) - t0) / 1e3,
                                                          sum(r['e'] <= chain[0]['e'] for r in ks), len(ks)))
    print('%-38s %8s %10.1f' % ('sum', '', total))
    d = sorted((r['e'] - r['s']) / 1e3 for r in chains)
    print('sampling chain over the %d steps of the trace: min %.1f  median %.1f  max %.1f us' % (len(d), d[0], d[len(d) // 2], d[-1]))


if __name__ == '__main__':
    main()
