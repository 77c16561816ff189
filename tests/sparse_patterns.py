"""Sparsity patterns that are not bundle-adjustment shaped, shared by the GPU parity tests (test_sparse_patterns_gpu.py)
and the CPU test that pins the symbolic phase bit for bit (test_library_cpu.py).  Every generator draws from the
generator it is given and leaves it where the caller goes on drawing values."""
import numpy as np


def rows_to_csc(rows, N):
    Jp = [0]
    Ji = []
    for r in rows:
        r = sorted(set(int(i) for i in r))
        Ji.extend(r)
        Jp.append(len(Ji))
    return np.array(Jp, dtype=np.int32), np.array(Ji, dtype=np.int32)


def random_structured_pattern(rng, scale=1):
    """variable blocks of random widths, a few of them 'dense' (touched by every row), rows drawn
    from a small set of templates and repeated 1..10 times (row-blocks), random values"""
    nblk = int(rng.integers(6, 40))*scale
    widths = rng.integers(1, 10, size=nblk)
    starts = np.concatenate([[0], np.cumsum(widths)])
    N = int(starts[-1])
    ndense = int(rng.integers(0, 3))
    dense_blocks = list(rng.choice(nblk, size=ndense, replace=False)) if ndense else []
    templates = []
    for _ in range(int(rng.integers(3, 60))*scale):
        k = int(rng.integers(1, min(5, nblk) + 1))
        blks = set(rng.choice(nblk, size=k, replace=False).tolist()) | set(dense_blocks)
        templates.append(sorted(blks))
    rows = []
    target = int(rng.integers(N + 20, 6 * N + 200))
    while len(rows) < target:
        t = templates[int(rng.integers(0, len(templates)))]
        idx = np.concatenate([np.arange(starts[b], starts[b + 1]) for b in t])
        for _ in range(int(rng.integers(1, 11))):
            rows.append(idx)
    # every block gets as many rows of its own as it is wide, so that J has full column rank
    # (the values of these rows are boosted by the caller)
    ntail = 0
    for b in range(nblk):
        for _ in range(int(widths[b])):
            rows.append(np.arange(starts[b], starts[b + 1]))
            ntail += int(widths[b])
    return N, rows, ntail


def ragged_rows(rng, seed):
    """(N, M, rows): rows of 1..9 entries, several runs of <= 2048 values, the last row of 1 + seed % 3 entries"""
    N = 120
    M = 3000 + seed          # several runs of <= 2048 values
    rows = [rng.choice(N, size=rng.integers(1, 10), replace=False) for _ in range(M)]
    rows[-1] = rows[-1][:1 + seed % 3]
    return N, M, rows
