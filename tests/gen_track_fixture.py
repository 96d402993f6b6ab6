"""Writes tests/golden/track_merge_*.npz: the REFERENCE's own multi_track_merge (utils/utils.py:343-397, reached through the
utils module its inference module imports) on generated reruns -- inputs and outputs.  Container-only, like tests/gen_occl_fixture.py.

    python tests/gen_track_fixture.py [OUT_DIR]

A file holds ids (K,) int64, track_col, abstract (K, M, 3 + E), features (K, D), outputs (K, N, G) float32 (already squashed
values: the merge's squash codes are all identity) and the reference's merged_abstract, merged_features, merged_output.
The reference asserts that the first three abstract columns agree across the reruns when K >= 3: the generator shares them.
The tracking scores are drawn from an adversarial pool (0.5 and its fp32 neighbours, equal scores in several reruns, +-0, 1,
NaN, a subnormal); rows 0 .. 3 of every case are set by hand: exactly 0.5, a tie at >= 0.5, everything below 0.5, a NaN followed
by a larger score.  The other channels hold some subnormal and +-0 values.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

# (K, N, G, track column, ids)
CASES = [
    (1, 64, 5, 4, [7]),
    (2, 257, 6, 4, [3, 1]),
    (3, 257, 6, 4, [4095, 0, 12]),
    (5, 1025, 5, 4, [9, 2, 4095, 0, 5]),
    (6, 300, 16, 15, [5, 4, 3, 2, 1, 0]),
    (7, 300, 29, 15, [100, 7, 4000, 1, 0, 33, 2]),
]
NAMES = ['track_merge_k%d_n%d_g%d' % c[:3] for c in CASES]
M, E, D = 24, 5, 32                            # abstract points, their feature columns, global feature size

HALF = np.float32(0.5)
SCORE_POOL = np.array([0.5, np.nextafter(HALF, np.float32(0)), np.nextafter(HALF, np.float32(1)), 0.75, 0.75, 0.0, -0.0, 1.0,
                       np.nan, 1e-40, 0.25, 0.9], dtype=np.float32)
OTHER_POOL = np.array([1e-40, -1e-40, 0.0, -0.0, 1.4e-45], dtype=np.float32)


def make_case(K, N, G, track_col, seed):
    rng = np.random.default_rng(seed)
    outputs = rng.uniform(0.0, 1.0, size=(K, N, G)).astype(np.float32)
    special = rng.uniform(size=(K, N, G)) < 0.1
    outputs[special] = OTHER_POOL[rng.integers(0, len(OTHER_POOL), size=int(special.sum()))]
    scores = SCORE_POOL[rng.integers(0, len(SCORE_POOL), size=(K, N))]
    mixed = rng.uniform(size=(K, N)) < 0.3                            # (ordinary scores among the pool's)
    scores[mixed] = rng.uniform(0.0, 1.0, size=int(mixed.sum())).astype(np.float32)
    scores[:, 0] = 0.25
    scores[K - 1, 0] = 0.5                                            # row 0: exactly 0.5 in the last rerun
    scores[:, 1] = 0.75                                               # row 1: a tie at >= 0.5 in every rerun
    scores[:, 2] = np.nextafter(HALF, np.float32(0))                  # row 2: everything below 0.5
    scores[:, 3] = 0.6
    scores[0, 3] = np.nan                                             # row 3: a NaN, then larger scores
    if K > 1:
        scores[1, 3] = 0.9
    outputs[:, :, track_col] = scores
    abstract = rng.normal(size=(K, M, 3 + E)).astype(np.float32)
    abstract[:, :, :3] = abstract[0, :, :3]
    abstract[:, 0, 3] = OTHER_POOL[:1]
    features = rng.normal(size=(K, D)).astype(np.float32)
    return abstract, features, outputs


def write(out_dir):
    from oracle import ref_import
    merge = ref_import.load().inference.utils.multi_track_merge        # (utils/utils.py, as eval/inference.py:265 calls it)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for name, (K, N, G, track_col, ids) in zip(NAMES, CASES):
        assert len(ids) == K and ids != sorted(ids) or K == 1
        abstract, features, outputs = make_case(K, N, G, track_col, 1000 + 10 * K + G)
        got = merge(list(ids), [a.copy() for a in abstract], [f.copy() for f in features], [o.copy() for o in outputs], track_col)
        merged_abstract, merged_features, merged_output = (np.asarray(a) for a in got)
        assert merged_output.dtype == np.float32 and merged_abstract.dtype == np.float32 and merged_features.dtype == np.float32
        path = os.path.join(out_dir, name + '.npz')
        np.savez_compressed(path, ids=np.asarray(ids, dtype=np.int64), track_col=np.int64(track_col), abstract=abstract,
                            features=features, outputs=outputs, merged_abstract=merged_abstract, merged_features=merged_features,
                            merged_output=merged_output)
        size = os.path.getsize(path)
        assert size < 480 * 1024, (path, size)
        paths.append((path, size))
    return paths


if __name__ == '__main__':
    for path, size in write(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'golden')):
        print('%8d  %s' % (size, path))
