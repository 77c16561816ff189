"""Patterns and the numpy restatements shared by tests/test_jacobian_check_{cpu,gpu}.py: nothing here calls the library."""
import numpy as np


def first_fit(N, M, Jp, Ji):
    """First-fit colouring in natural variable order, restated: v takes the smallest colour that no already-coloured
    variable sharing a row with it holds; a variable in no row gets 0.  Returns colour[N]."""
    rows_of = [[] for _ in range(N)]
    for r in range(M):
        for v in Ji[Jp[r]:Jp[r + 1]]:
            rows_of[v].append(r)
    colour = np.full(N, -1, dtype=np.int32)
    for v in range(N):
        taken = set()
        for r in rows_of[v]:
            for u in Ji[Jp[r]:Jp[r + 1]]:
                if colour[u] >= 0:
                    taken.add(int(colour[u]))
        c = 0
        while c in taken:
            c += 1
        colour[v] = c
    return colour


def max_neighbours(N, M, Jp, Ji):
    """the largest number of distinct other variables a variable shares a row with"""
    nb = [set() for _ in range(N)]
    for r in range(M):
        vs = [int(v) for v in Ji[Jp[r]:Jp[r + 1]]]
        for v in vs:
            nb[v].update(vs)
    return max((len(s - {v}) for v, s in enumerate(nb)), default=0)


def ragged_pattern(N=40, M=70, seed=11, empty_row=13, lonely_var=29):
    """1 to 5 entries a row, row `empty_row` empty, variable `lonely_var` in no row: (Jp, Ji) of Jt, row indices ascending"""
    rng = np.random.default_rng(seed)
    others = np.array([v for v in range(N) if v != lonely_var])
    Jp, Ji = [0], []
    for r in range(M):
        k = 0 if r == empty_row else int(rng.integers(1, 6))
        Ji.extend(sorted(rng.choice(others, size=k, replace=False).tolist()))
        Jp.append(len(Ji))
    return np.array(Jp, dtype=np.int32), np.array(Ji, dtype=np.int32)


def full_pattern(M, N):
    """every variable in every row: a dense problem as a sparse one"""
    return (np.arange(M + 1, dtype=np.int32) * N), np.tile(np.arange(N, dtype=np.int32), M)


def model(Jp, Ji, a, pstar, eps, p):
    """x, u and the Jacobian values of problems/device_gradcheck_problems.hip's sparse model at p"""
    M = len(Jp) - 1
    row = np.repeat(np.arange(M), np.diff(Jp))
    u = np.zeros(M)
    np.add.at(u, row, a * (p[Ji] - pstar[Ji]))
    return u + eps * np.sin(u), u, a * (1.0 + eps * np.cos(u))[row]
