"""The shapes at which tests/test_dense_shapes_gpu.py runs the single-problem dense path (DLG_DENSE, DLG_DENSE_PRODUCTS:
kernels_dense.hip, dense_diag.hip), the long-double references of its operations and the rounding bounds they are held to;
tests/test_dense_shapes_cpu.py asserts all of it without a GPU.  Test infrastructure: numpy, tests/exact_ei.py and the CPU
oracle; nothing of the library under test computes a number in here.

References: np.longdouble (x87 extended, 64-bit significand: unit roundoff 2^-64, 2048 times below a double's) from the
same float64 J and x that go to the device.  Bounds: first-order rounding bounds in units of U = 2^-53, evaluated in long
double from the absolute values of the operands; no tolerance in here was read off a run of the code under test.
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

from libdogleg_amd.ctypes_defs import CB_DENSE, CB_PRODUCTS        # (the callback types of the C-ABI: definitions, no code)

LD = np.longdouble
LD_EPS_NEEDED = 1e-18                    # the references stand 2^11 below the bounds only on an extended-precision long double


def require_long_double():
    assert np.finfo(LD).eps < LD_EPS_NEEDED, (
        f"np.longdouble has eps {np.finfo(LD).eps}: no extended precision on this platform -- the references of "
        "tests/dense_shapes.py need it and do not fall back to float64")


U = LD(2) ** -53                         # unit roundoff of the device's arithmetic


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------- restated from libdogleg_amd/csrc/kernels_dense.hip
TPB = 256                                # kernels_dense.hip:30   constexpr int TPB = 256;
KC = 16                                  # kernels_dense.hip:206  constexpr int KC = 16;
SYRK_WT = 64                             # kernels_dense.hip      dense_factorize: launch_syrk<64>(... true, b->slabs ...)
BT = 2 * SYRK_WT                         # kernels_dense.hip:213  constexpr int BT = 2*WT;  (128 for the JtJ SYRK)
SUPER = 4                                # kernels_dense.hip:236  constexpr int S = 4;  (side of a super-tile, in block tiles)
GROUP = 8                                # kernels_dense.hip:233  const int r = pos & 7, q = pos >> 3;
SYRK_RSUB = 8                            # kernels_dense.hip:367  constexpr int SYRK_RSUB = 8;
NB = 64                                  # kernels_dense.hip:421, dense_diag.hip:9  constexpr int NB = 64;
STEP_REM_WIDE = 1024                     # kernels_dense.hip      potrf_lower: if(rem >= 1024) launch_syrk<64> else <32>
EVAL_RPC0, EVAL_RPC_MIN, EVAL_WG = 128, 16, 2048    # dense_eval: int rpc = 128; while(rpc > 16 && chunks*colblocks < 2048) rpc >>= 1;
EVAL_TWO_STAGE = 64                      # dense_eval: nsl = (nchunks >= 64) ? 32 : 0
NORM2_G_MAX, NORM2_WAVES = 2048, 4       # dense_norm2_Jv: g = cdiv(M, 4); if(g > 2048) g = 2048;
# ---------------------------------------------------------------- restated from libdogleg_amd/csrc/dense_diag.hip
FOLD_FWD_FROM = 8                        # k_trsv_tiles: const bool ffold = i >= 8;
FOLD_BWD_WITHIN = 8                      # k_trsv_tiles: const bool b_early = T - 1 - i < 8;
NCU = 256                                # MI355X; dense_solve: if(T >= 2 && T <= b->ncu/2 && !b->knobs.trsv_steps)


def tiles(N):
    """T of run_potrf / dense_solve: 64-column tiles"""
    return cdiv(N, NB)


def last_tile(N):
    """columns of the last 64-column tile"""
    return N - (tiles(N) - 1) * NB


def one_launch_potrf(N):
    """run_potrf: if(!b->knobs.potrf_steps && T >= 2) k_potrf_tiles"""
    return tiles(N) >= 2


def one_launch_trsv(N, ncu=NCU):
    return 2 <= tiles(N) <= ncu // 2


def trsv_regime(N):
    """which paths of k_trsv_tiles the block rows i = 0 .. T - 1 take, from ffold = i >= 8 (two products folded ahead on the
    way down) and b_early = T - 1 - i < 8 (the products of the way back formed before the way down):
      'single'  T = 1: the step form;
      'plain'   T <= 8: no row folds ahead, every row is early on the way back;
      'fold'    9 <= T <= 16: rows i >= 8 fold ahead and every one of them is early on the way back too; the rows
                i <= T - 9 take neither early path;
      'fold+'   T >= 17: rows 8 .. T - 9 fold ahead on the way down and are NOT early on the way back -- all four
                combinations occur"""
    T = tiles(N)
    if T < 2:
        return "single"
    rows = {(i >= FOLD_FWD_FROM, T - 1 - i < FOLD_BWD_WITHIN) for i in range(T)}
    if (True, False) in rows:
        return "fold+"
    return "fold" if (True, True) in rows else "plain"


def block_tiles(N):
    """T of launch_syrk<64>: 128-row block tiles of the JtJ SYRK"""
    return cdiv(N, BT)


def last_block_tile(N):
    return N - (block_tiles(N) - 1) * BT


def super_tiles(N):
    """TS of k_syrk_lower: super-tiles of 4 x 4 block tiles along a side"""
    return cdiv(block_tiles(N), SUPER)


def group_sizes(ntiles):
    """positions of a split that share pos & 7: k_syrk_lower's `(ntl - x + 7) >> 3`"""
    return [(ntiles - x + 7) >> 3 for x in range(GROUP)]


def syrk_nsplit(ntiles, K, resident=512):
    """kernels_dense.hip: static int syrk_nsplit(int ntiles, int K, int resident = 512)"""
    nom = cdiv(1536, ntiles)
    maxs = K // (4 * KC)
    nom = max(1, min(nom, maxs))
    lo = max(1, 2 * nom // 3)
    hi = max(lo, min(max(maxs, 1), nom + nom // 2 + 1))

    def eff(ns):
        r = ntiles * ns / resident
        return r / np.ceil(r)
    best = max(eff(ns) for ns in range(lo, hi + 1))
    for ns in range(lo, hi + 1):
        if eff(ns) >= best - 0.03:
            return ns
    return nom


def syrk_split(N, M):
    """(ks, kper, empty splits) of launch_syrk<64>(overwrite = true): ks = max(2, syrk_nsplit), kper = max(KC,
    cdiv(cdiv(K, ks), KC)*KC).  (dense_create sizes the slabs with the same ks: the `while(per*ks > ws_bytes)` never bites)"""
    Tb = block_tiles(N)
    ks = max(2, syrk_nsplit(Tb * (Tb + 1) // 2, M))
    kper = max(KC, cdiv(cdiv(M, ks), KC) * KC)
    return ks, kper, sum(1 for s in range(ks) if s * kper >= M)


def eval_chunks(M, N):
    """(rows per chunk, chunks, two-stage column sums) of dense_eval"""
    rpc = EVAL_RPC0
    while rpc > EVAL_RPC_MIN and cdiv(M, rpc) * cdiv(N, TPB) < EVAL_WG:
        rpc >>= 1
    n = cdiv(M, rpc)
    return rpc, n, n >= EVAL_TWO_STAGE


def norm2_rows_per_wave(M):
    """most rows a wave of k_norm2_Jv_part takes: g = min(2048, cdiv(M, 4)) workgroups of 4 waves"""
    g = max(1, min(NORM2_G_MAX, cdiv(M, NORM2_WAVES)))
    return cdiv(M, NORM2_WAVES * g)


def step_form_rems(N):
    """the trailing sizes rem = n - kb - nb of potrf_lower, one per 64-column step that has rows below it"""
    return [N - kb - min(NB, N - kb) for kb in range(0, N, NB) if N - kb - min(NB, N - kb) > 0]


# ---------------------------------------------------------------- the cases
LAMBDAS = (0.0, 1e-10, 1.0)


M_FLOOR = 515


def default_M(N):
    """2 N + 3: odd and not a multiple of 16 -- but 515 (odd, 3 past a multiple of 16) at least: a Gaussian J with only
    twice as many rows as columns has c of 80 - 150 for N <= 192 (the 64 x 64 blocks of its factor are what is badly
    conditioned then), and c <= C_MAX is the condition the inputs have to meet"""
    return max(2 * N + 3, M_FLOOR)


# N: (T, columns of the last tile, block tiles, rows of the last block tile, super-tiles, the regime of k_trsv_tiles)
N_CASES = {
    1: (1, 1, 1, 1, 1, "single"),          # T = 1: the step form even by default; one column
    2: (1, 2, 1, 2, 1, "single"),          # the smallest N with an off-diagonal entry; a pair of rows in k_syrk_reduce
    15: (1, 15, 1, 15, 1, "single"),       # one short of an MFMA tile of 16
    16: (1, 16, 1, 16, 1, "single"),       # exactly one MFMA tile
    17: (1, 17, 1, 17, 1, "single"),       # one past it; odd: the last row of k_syrk_reduce's pair loop stands alone
    63: (1, 63, 1, 63, 1, "single"),       # one short of the 64-column tile
    64: (1, 64, 1, 64, 1, "single"),       # exactly one tile: the largest N in the step form by default
    65: (2, 1, 1, 65, 1, "plain"),         # the smallest N in k_potrf_tiles / k_trsv_tiles: a last tile of ONE column
    127: (2, 63, 1, 127, 1, "plain"),      # one short of two tiles and of the 128-row block tile
    128: (2, 64, 1, 128, 1, "plain"),      # two whole tiles, one whole block tile
    129: (3, 1, 2, 1, 1, "plain"),         # a third tile and a second block tile of one row
    191: (3, 63, 2, 63, 1, "plain"),
    192: (3, 64, 2, 64, 1, "plain"),       # three whole tiles
    193: (4, 1, 2, 65, 1, "plain"),
    255: (4, 63, 2, 127, 1, "plain"),
    256: (4, 64, 2, 128, 1, "plain"),      # two whole block tiles
    257: (5, 1, 3, 1, 1, "plain"),
    512: (8, 64, 4, 128, 1, "plain"),      # T = 8: the last T at which no block row folds ahead; 4 block tiles: ONE super-tile
    513: (9, 1, 5, 1, 2, "fold"),          # T = 9: row 8 folds ahead, row 0 takes neither early path; 5 block tiles: a second super-tile of one block tile
    1024: (16, 64, 8, 128, 2, "fold"),     # T = 16: the last T at which every row that folds ahead is early on the way back; 2 x 2 whole super-tiles
    1025: (17, 1, 9, 1, 3, "fold+"),       # T = 17: row 8 folds ahead but is not early on the way back; a third super-tile
    1089: (18, 1, 9, 65, 3, "fold+"),      # the step form only: its first trailing update has rem = 1025 >= 1024 -> launch_syrk<64>
}
STEP_FORM_ONLY = (1089,)
ORACLE_AGREEMENT_MAX_N = 513             # the project's own 1e-10 agreement with orc_step_dense is kept up to here

# the M sweep: lambda = 1.0, so that M < N still factorises; J Gaussian with sigma = 1/8, so that lambda dominates J'J
# where M < N (sigma = 1: c of 150 - 630 for M = 15 .. 129; c <= C_MAX is the condition on the inputs)
M_SWEEP_N = (65, 129)
M_SWEEP_LAMBDA = 1.0
M_SWEEP_SIGMA = 0.125
# M: (ks, kper, empty splits) of the SYRK at N = 65 / at N = 129 where it differs, (rows per chunk, chunks, two-stage sums)
# of dense_eval (one column block of 256 at both N)
M_SWEEP = {
    1: ((2, 16, 1), (16, 1, False)),          # one row: one K-chunk of one row, the second split empty
    15: ((2, 16, 1), (16, 1, False)),         # one short of KC
    16: ((2, 16, 1), (16, 1, False)),         # exactly KC: the second split still empty
    17: ((2, 16, 0), (16, 2, False)),         # one past: the second split holds ONE row; a second chunk of one row
    63: ((2, 32, 0), (16, 4, False)),         # maxs = K/(4 KC) = 0
    64: ((2, 32, 0), (16, 4, False)),         # maxs = 1
    65: ((2, 48, 0), (16, 5, False)),         # kper rounds up to 3 KC: the second split holds 17 rows
    127: ((2, 64, 0), (16, 8, False)),
    128: ((2, 64, 0), (16, 8, False)),        # maxs = 2: the first K at which syrk_nsplit itself may say 2
    129: ((2, 80, 0), (16, 9, False)),
    1008: ((10, 112, 1), (16, 63, False)),    # 63 chunks: the other side of `nchunks >= 64`; the tenth split is empty
    1023: ((10, 112, 0), (16, 64, True)),     # 64 chunks (the last of 15 rows): two-stage column sums
    1024: {65: ((10, 112, 0), (16, 64, True)), 129: ((11, 96, 0), (16, 64, True))},      # 64 whole chunks
    1025: {65: ((10, 112, 0), (16, 65, True)), 129: ((11, 96, 0), (16, 65, True))},      # a 65th chunk of one row
}
# rows per wave of k_norm2_Jv_part above 1: N = 3 only (J stays small), sigma = 1; M: rows per wave
M_SWEEP_LONG_N = 3
M_SWEEP_LONG = {8191: 1, 8192: 1, 8193: 2}


def m_sweep_claim(N, M):
    v = M_SWEEP[M]
    return v[N] if isinstance(v, dict) else v


# lambda on the diagonal: sum_k L_ik^2 at lambda = 1e-10 against lambda = 0, row by row.  The bound on a row sum is
# relative to J'J's diagonal (diag_rows_bound), lambda is absolute: J is scaled by 2^-6 (exactly: the same roundings, entry
# for entry, as the unscaled problem) so that (J'J)_ii ~ M / 4096 <= 0.6 and the two bounds together stay below
# DIAG_SHARP lambda at every N -- a lambda missing from one diagonal entry is then 1 / DIAG_SHARP times its bound
DIAG_SIGMA = 2.0 ** -6
DIAG_LAMBDA = 1e-10
DIAG_SHARP = 0.5

PRODUCTS_N = (64, 65, 129, 257)
PRODUCTS_LAMBDAS = (0.0, 1e-10)

# c = 4 max_j || |L_jj^-1| |L_jj| ||_inf over the 64 x 64 diagonal blocks of the long-double factor, the largest over
# LAMBDAS, per N at M = default_M(N) (block_c below; plain Gaussian J: c <= C_MAX is a condition on the inputs)
C_MAX = 64.0
C_RECORDED = {1: 4.0, 2: 4.3, 15: 8.6, 16: 11.3, 17: 10.2, 63: 35.4, 64: 38.7, 65: 36.6, 127: 42.4, 128: 40.5, 129: 38.5,
              191: 44.1, 192: 45.2, 193: 48.3, 255: 57.4, 256: 55.5, 257: 49.4, 512: 35.7, 513: 32.8, 1024: 22.8, 1025: 22.3,
              1089: 22.2}


# ---------------------------------------------------------------- inputs
# The factor's bound c gamma |L||L'| (check_factor) is the Cholesky factorisation's own; for the part of the error that
# the SYRK contributes, gamma_M (|J|'|J|)_ij, it is a theorem only where (|L||L'|)_ij is not far below (|J|'|J|)_ij.  In
# column 0, (|L||L'|)_i0 = |A_i0|, and where a Gaussian draw leaves that entry a thousand times below its typical size a
# correct float64 SYRK exceeds the bound at c = 1 (seen: 1.45 times at N = 127, 159 times at 1100 x 513).  As tests/dense_batch_shapes.py does with
# its decision margins, the draw is chosen from what the REFERENCE says: the first seed at which the oracle's float64
# route meets every bound at c = 1 (test_dense_shapes_cpu.py asserts that it does).  (N, M, zero columns): seed shift;
# shapes not listed: 0.  The device's c is 4 to 55: an entry like that stands at a quarter of its bound at most.
SEED_SHIFT = {
    (127, 515, ()): 1, (129, 515, ()): 1, (191, 515, ()): 1, (192, 515, ()): 4, (255, 515, ()): 1, (256, 515, ()): 1,
    (257, 517, ()): 3, (512, 1027, ()): 3, (1024, 2051, ()): 17, (1025, 2053, ()): 6, (1089, 2181, ()): 1,
    (65, 64, ()): 1, (65, 128, ()): 1, (65, 129, ()): 3, (65, 1023, ()): 1, (65, 1025, ()): 2, (129, 15, ()): 2,
    (129, 16, ()): 2, (129, 63, ()): 1, (129, 64, ()): 1, (129, 127, ()): 1, (129, 128, ()): 1, (129, 1008, ()): 1,
    (129, 1023, ()): 2, (130, 515, (63,)): 1, (130, 515, (129,)): 1, (193, 400, (70, 192)): 1, (257, 600, (128, 256)): 1,
    (257, 600, (63,)): 1, (513, 1100, (0,)): 2, (513, 1100, (64,)): 6, (513, 1100, (63, 512)): 6,
}
def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


@functools.lru_cache(maxsize=64)
def inputs(N, M, zero=(), alt=0, sigma=1.0):
    """(x, J, p): plain Gaussian J (M x N, row-major), x, p, seeded by the shape; `zero`: columns of J set to exactly 0;
    alt: another draw of the same shape"""
    rng = _rng(N, M, alt + SEED_SHIFT.get((N, M, tuple(zero)), 0))
    J = sigma * rng.standard_normal((M, N))
    x = rng.standard_normal(M)
    p = rng.standard_normal(N)
    for c in zero:
        J[:, c] = 0.0
    return x, np.ascontiguousarray(J), p


# ---------------------------------------------------------------- long-double linear algebra
_THREADS = max(1, min(8, os.cpu_count() or 1))


def gram_lower(X, Y=None, blk=64):
    """tril(X Y') in long double for X, Y of shape (n, k) with contiguous rows.  Block rows go to threads: numpy's
    long-double loops run without the interpreter lock, and they have no BLAS behind them"""
    Y = X if Y is None else Y
    n = X.shape[0]
    out = np.zeros((n, n), dtype=LD)

    def job(b):
        e = min(n, b + blk)
        out[b:e, :e] = X[b:e] @ Y[:e].T
    with ThreadPoolExecutor(_THREADS) as ex:
        list(ex.map(job, range(0, n, blk)))
    return np.tril(out)


def cholesky(A):
    """the Cholesky factor of the symmetric matrix whose lower triangle is A (long double), column by column with
    vectorised updates; (L, -1), or (None, j) at the first pivot j that is not positive"""
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            return None, j
        L[j:, j] = v / np.sqrt(v[0])
    return L, -1


def solve_lower(L, b, transposed=False):
    """L y = b, or L' y = b, by substitution in long double"""
    n = len(b)
    y = np.array(b, dtype=LD)
    if not transposed:
        for i in range(n):
            y[i] = (y[i] - L[i, :i] @ y[:i]) / L[i, i]
    else:
        for i in range(n - 1, -1, -1):
            y[i] = (y[i] - L[i + 1:, i] @ y[i + 1:]) / L[i, i]
    return y


def sym_matvec(Alow, v):
    """(the symmetric matrix of the lower triangle Alow) v"""
    return Alow @ v + np.tril(Alow, -1).T @ v


def block_c(L):
    """4 max_j || |L_jj^-1| |L_jj| ||_inf over the NB x NB diagonal blocks: the kernels multiply by the inverses of these
    blocks where a substitution would be backward stable outright; the product is so only up to their conditioning"""
    worst = LD(0)
    for j0 in range(0, L.shape[0], NB):
        B = L[j0:j0 + NB, j0:j0 + NB]
        n = B.shape[0]
        X = np.zeros((n, n), dtype=LD)
        for i in range(n):
            e = np.zeros(n, dtype=LD)
            e[i] = 1
            X[i] = (e - B[i, :i] @ X[:i]) / B[i, i]
        worst = max(worst, np.max(np.sum(np.abs(X) @ np.abs(B), axis=1)))
    return float(4 * worst)


# ---------------------------------------------------------------- the references
@functools.lru_cache(maxsize=6)
def _gram1(N, M, zero=(), alt=0):
    x, J, p = inputs(N, M, zero, alt)
    return gram_lower(np.ascontiguousarray(J.T).astype(LD))


def _gram(N, M, zero=(), alt=0, sigma=1.0):
    """tril(J'J) in long double; sigma: a power of two -- J = sigma G exactly, so J'J = sigma^2 G'G exactly"""
    assert np.frexp(sigma)[0] == 0.5
    return _gram1(N, M, zero, alt) * LD(sigma) ** 2


@functools.lru_cache(maxsize=6)
def point(N, M, zero=(), alt=0, sigma=1.0):
    """what K1 / K3 are held to: Jtx, |J|'|x|, |x|^2, max |Jtx| in long double"""
    require_long_double()
    x, J, p = inputs(N, M, zero, alt, sigma)
    xl = x.astype(LD)
    if M * N <= 1 << 18:
        Jl = J.astype(LD)
        g, gabs = Jl.T @ xl, np.abs(Jl).T @ np.abs(xl)
    else:                                  # (column blocks of J' in threads, as gram_lower)
        Jt = np.ascontiguousarray(J.T).astype(LD)
        g, gabs = np.zeros(N, dtype=LD), np.zeros(N, dtype=LD)

        def job(b):
            g[b:b + 64] = Jt[b:b + 64] @ xl
            gabs[b:b + 64] = np.abs(Jt[b:b + 64]) @ np.abs(xl)
        with ThreadPoolExecutor(_THREADS) as ex:
            list(ex.map(job, range(0, N, 64)))
    return SimpleNamespace(x=x, J=J, p=p, N=N, M=M, g=g, gabs=gabs, n2x=xl @ xl, gmax=np.max(np.abs(g)))


@functools.lru_cache(maxsize=12)
def reference(N, M, lam, zero=(), alt=0, sigma=1.0):
    """point() + A = J'J + lam I (lower), its factor L (None where a pivot fails, `bad` the pivot), c and the Gauss-Newton
    step gn = -A^-1 J'x with its squared norm"""
    P = point(N, M, zero, alt, sigma)
    A = _gram(N, M, zero, alt, sigma).copy()
    A[np.diag_indices(N)] += LD(lam)
    L, bad = cholesky(A)
    r = SimpleNamespace(**vars(P), lam=lam, A=A, L=L, bad=bad, c=None, gn=None, n2gn=None)
    if L is not None:
        r.c = block_c(L)
        r.gn = -solve_lower(L, solve_lower(L, P.g), transposed=True)
        r.n2gn = r.gn @ r.gn
    return r


def products_reference(N, M, lam, packed, neg=None):
    """the products form of the same problem: norm2x, Jtx, JtJ are the long-double products ROUNDED to float64 -- those
    doubles are the inputs of the device and of this reference alike.  neg = (k, value): entry (k, k) of JtJ replaced.
    Returns the namespace of reference() with A built from the rounded JtJ, plus n2x64, g64, H64 (the full symmetric
    float64 matrix) and the array `upload` in the storage form asked for"""
    zero = () if neg is None else (neg[0],)
    P = point(N, M, zero)
    G = _gram(N, M, zero)
    H64 = (G + np.tril(G, -1).T).astype(np.float64)
    if neg is not None:
        H64[neg[0], neg[0]] = neg[1]
    g64 = P.g.astype(np.float64)
    A = np.tril(H64).astype(LD)
    A[np.diag_indices(N)] += LD(lam)
    L, bad = cholesky(A)
    r = SimpleNamespace(N=N, M=M, p=P.p, lam=lam, A=A, L=L, bad=bad, c=None, gn=None, n2gn=None, g=g64.astype(LD),
                        n2x64=float(P.n2x), g64=g64, H64=H64,
                        upload=H64[np.triu_indices(N)].copy() if packed else H64.copy())
    if L is not None:
        r.c = block_c(L)
        r.gn = -solve_lower(L, solve_lower(L, r.g), transposed=True)
        r.n2gn = r.gn @ r.gn
    return r


def unpack_factor(fac, N):
    """dlg_factor_download_dense's packed array (column-major packed lower == row-major packed upper of L') -> L"""
    Lt = np.zeros((N, N))
    Lt[np.triu_indices(N)] = fac
    return np.ascontiguousarray(Lt.T)


# ---------------------------------------------------------------- the bounds: each returns max(observed / bound)
def _ratio(obs, bound):
    """the largest observed / bound; an entry whose bound is 0 must be 0 itself"""
    obs, bound = np.atleast_1d(np.abs(np.asarray(obs, dtype=LD))), np.atleast_1d(np.asarray(bound, dtype=LD))
    r = np.where(bound > 0, obs / np.where(bound > 0, bound, 1), np.where(obs == 0, 0, np.inf))
    return float(np.max(r)) if r.size else 0.0


def sum_bound(k, abs_terms):
    """a sum of k terms (products included), in any order, fused or not: |fl(sum) - sum| <= (k + 1) U sum|terms| + O(U^2)
    (one rounding per product, k - 1 per addition chain at worst); stated as 4 (k + 2) U sum|terms|: the factor 4 is the
    margin for the second-order terms and for the scalar arithmetic behind the sum"""
    return 4 * (k + 2) * U * np.asarray(abs_terms, dtype=LD)


def check_eval(P, jtx, n2x, gmax):
    """K1: ratios for Jtx (componentwise, M terms each), |x|^2 (M terms), max |Jtx| (|max a - max b| <= max |a - b|)"""
    bg = sum_bound(P.M, P.gabs)
    return dict(jtx=_ratio(jtx.astype(LD) - P.g, bg), norm2x=_ratio(LD(n2x) - P.n2x, sum_bound(P.M, P.n2x)),
                gmax=_ratio(LD(gmax) - P.gmax, np.max(bg)))


def cauchy_reference(P, g_dev):
    """K3 from the Jtx the device holds (g_dev, taken as exact input): kappa = -|g|^2 / |J g|^2, cauchy = kappa g,
    |cauchy|^2 = kappa^2 |g|^2, with first-order bounds:
      |g|^2: N terms; (J g)_r: N terms, e_r = sum_bound(N, |J_r| |g|); |J g|^2: M terms of squares that each carry
      2 |(J g)_r| e_r  ->  d(Jg2) = 2 |Jg| . e + sum_bound(M, Jg2);
      kappa: relative d(g2)/g2 + d(Jg2)/Jg2 (the division's rounding is in the margin of sum_bound);
      cauchy_i: |g_i| d(kappa) + 4 U |kappa g_i|;  |cauchy|^2 = kappa^2 g2: 2 |kappa| g2 d(kappa) + kappa^2 d(g2)"""
    g = g_dev.astype(LD)
    Jl = P.J.astype(LD) if P.M * P.N <= 1 << 21 else None
    if Jl is not None:
        Jg, Jga = Jl @ g, np.abs(Jl) @ np.abs(g)
    else:
        Jg, Jga = np.zeros(P.M, dtype=LD), np.zeros(P.M, dtype=LD)

        def job(b):
            blk = P.J[b:b + 128].astype(LD)
            Jg[b:b + 128] = blk @ g
            Jga[b:b + 128] = np.abs(blk) @ np.abs(g)
        with ThreadPoolExecutor(_THREADS) as ex:
            list(ex.map(job, range(0, P.M, 128)))
    g2, Jg2 = g @ g, Jg @ Jg
    dg2 = sum_bound(P.N, g2)
    dJg2 = 2 * (np.abs(Jg) @ sum_bound(P.N, Jga)) + sum_bound(P.M, Jg2)
    k = -g2 / Jg2
    dk = np.abs(k) * (dg2 / g2 + dJg2 / Jg2)
    return SimpleNamespace(k=k, cauchy=k * g, n2c=k * k * g2, d_cauchy=np.abs(g) * dk + 4 * U * np.abs(k * g),
                           d_n2c=2 * np.abs(k) * g2 * dk + k * k * dg2 + 4 * U * k * k * g2)


def check_cauchy(P, g_dev, cauchy, n2c):
    R = cauchy_reference(P, g_dev)
    return dict(cauchy=_ratio(cauchy.astype(LD) - R.cauchy, R.d_cauchy), norm2_cauchy=_ratio(LD(n2c) - R.n2c, R.d_n2c))


def abs_LLt_lower(Lf):
    """tril(|L| |L'|) in long double for a float64 or long-double factor"""
    return gram_lower(np.abs(np.ascontiguousarray(Lf)).astype(LD))


def check_factor(R, Lf, c):
    """|L L' - (J'J + lam I)| <= c gamma |L| |L'| on the lower triangle, gamma = (M + N + 2) U: M products per entry of the
    SYRK and up to N per entry of the factorisation, the standard componentwise bound of a Cholesky factorisation
    (gamma_{n+1} |L||L'|) carried over to a factor that was formed from a rounded J'J; L: the factor under test"""
    Ll = np.ascontiguousarray(Lf).astype(LD)
    gamma = (R.M + R.N + 2) * U
    return _ratio(gram_lower(Ll) - R.A, LD(c) * gamma * abs_LLt_lower(Lf))


def check_gn(R, Lf, gn, c):
    """|(J'J + lam I) gn + J'x| <= c gamma3 (|L| |L'| |gn|) componentwise, gamma3 = (M + 3 N + 2) U: the factor's bound
    plus N products in each of the two triangular solves"""
    gl = gn.astype(LD)
    La = np.abs(np.ascontiguousarray(Lf)).astype(LD)
    bound = LD(c) * (R.M + 3 * R.N + 2) * U * (La @ (La.T @ np.abs(gl)))
    return _ratio(sym_matvec(R.A, gl) + R.g, bound)


def check_norm2(v, n2):
    """a squared norm of the device's own vector: len(v) terms"""
    s = v.astype(LD) @ v.astype(LD)
    return _ratio(LD(n2) - s, sum_bound(len(v), s))


def diag_rows_bound(R0, Lf):
    """for the check of lambda on the diagonal: sum_k L_ik^2 of a device factor is row i of L L', so by check_factor's
    bound it lies within c gamma (|L||L'|)_ii = c gamma sum_k L_ik^2 of A_ii; two factors (lambda = 0 and 1e-10) -> the
    difference of their row sums is lambda to within the sum of their two bounds.  Returns (row sums, bound per row)
    for ONE factor; c of the lambda = 0 reference R0"""
    Ll = np.ascontiguousarray(Lf).astype(LD)
    s = np.sum(Ll * Ll, axis=1)
    return s, LD(R0.c) * (R0.M + R0.N + 2) * U * s


def step_reference(kind, a_dev, b_dev, n2c_dev, tr):
    """K7 from the vectors the device holds (cauchy a, Gauss-Newton b, |cauchy|^2 as it reported it), per kind
    (0 Cauchy to the edge: tr / sqrt(n2c) a; 1 Gauss-Newton: b; 2 interpolated: a + k (b - a) with
    k = (negc + sqrt(negc^2 - l2 (n2c - tr^2))) / l2, l2 = |a - b|^2, negc = <a - b, a>): (step, bound per entry, k, d(k))
      kind 0: two roundings of the scale, one of the product: 4 . 3 U |step_i|;  kind 1: a copy: 0;
      kind 2: d = a - b carries U |d| per entry; l2, negc: N terms each (the entries' own rounding doubles the terms:
      sum_bound over 2 N); disc = negc^2 - l2 (n2c - tr^2): 2 |negc| d(negc) + |n2c - tr^2| d(l2) + 4 U (negc^2 +
      |l2 (n2c - tr^2)|); k: (d(negc) + d(disc) / (2 sqrt disc)) / l2 + |k| d(l2) / l2 + 4 U |k|;
      step_i: |b_i - a_i| d(k) + 4 . 3 U (|a_i| + |k| |b_i - a_i|)"""
    a, b = a_dev.astype(LD), b_dev.astype(LD)
    n2c, tr = LD(n2c_dev), LD(tr)
    n = len(a)
    if kind == 0:
        s = tr / np.sqrt(n2c) * a
        return s, 12 * U * np.abs(s), None, None
    if kind == 1:
        return b, np.zeros(n, dtype=LD), None, None
    d = a - b
    l2, negc = d @ d, d @ a
    dl2, dnegc = sum_bound(2 * n, l2), sum_bound(2 * n, np.abs(d) @ np.abs(a))
    w = n2c - tr * tr
    disc = negc * negc - l2 * w
    assert disc > 0
    ddisc = 2 * np.abs(negc) * dnegc + np.abs(w) * dl2 + 4 * U * (negc * negc + np.abs(l2 * w))
    k = (negc + np.sqrt(disc)) / l2
    dk = (dnegc + ddisc / (2 * np.sqrt(disc))) / l2 + np.abs(k) * dl2 / l2 + 4 * U * np.abs(k)
    s = a + k * (b - a)
    return s, np.abs(b - a) * dk + 12 * U * (np.abs(a) + np.abs(k) * np.abs(b - a)), k, dk


def ei_bound(P, g_dev, step):
    """K8 = -2 <g, step> - |J step|^2 from the device's Jtx and step.  Against the value of exact arithmetic on J, x, step:
      <g, step>: g carries check_eval's bound e_g: e_g . |step|, + N terms: sum_bound(N, |g| . |step|);
      |J step|^2: as |J g|^2 in cauchy_reference;  the factor 2 and the subtraction: in the margin of sum_bound"""
    s = step.astype(LD)
    Jl = P.J.astype(LD) if P.M * P.N <= 1 << 21 else None
    if Jl is not None:
        Js, Jsa = Jl @ s, np.abs(Jl) @ np.abs(s)
    else:
        Js, Jsa = np.zeros(P.M, dtype=LD), np.zeros(P.M, dtype=LD)

        def job(b):
            blk = P.J[b:b + 128].astype(LD)
            Js[b:b + 128] = blk @ s
            Jsa[b:b + 128] = np.abs(blk) @ np.abs(s)
        with ThreadPoolExecutor(_THREADS) as ex:
            list(ex.map(job, range(0, P.M, 128)))
    inner = 2 * (sum_bound(P.M, P.gabs) @ np.abs(s) + sum_bound(P.N, np.abs(g_dev.astype(LD)) @ np.abs(s)))
    quad = 2 * (np.abs(Js) @ sum_bound(P.N, Jsa)) + sum_bound(P.M, Js @ Js)
    return float(-2 * (P.g @ s) - Js @ Js), inner + quad


def ei_products_bound(R, step):
    """the products form: -2 <g, step> - step' H step; g, H the uploaded doubles (exact inputs).  N terms; N rows of N
    terms, each row's sum then one of N terms of the outer sum: sum_bound(N, .) on both levels -> 2 sum_bound(N, |s|'|H||s|)
    (the packed form doubles the off-diagonal terms instead of visiting them twice: the same absolute sum)"""
    s = step.astype(LD)
    H = R.H64.astype(LD)
    val = -2 * (R.g @ s) - s @ (H @ s)
    return float(val), 2 * sum_bound(R.N, np.abs(R.g) @ np.abs(s)) + 2 * sum_bound(R.N, np.abs(s) @ (np.abs(H) @ np.abs(s)))


# ---------------------------------------------------------------- a pivot that fails inside the one-launch factorisation
# J with exactly-zero columns: J'J has exactly-zero rows and columns there, the problem decouples, and the step is well
# conditioned at lambda = 1e-10.  name: (N, M, zero columns) -- the column at 0, at 63 (the last of tile 0), at 64 (the
# first of tile 1), at N - 1 (a last tile of 1, 2 and 1 columns), and in two tiles at once.  M: 515 for N <= 130 (c <= C_MAX,
# as default_M)
ZERO_CASES = {
    "65-c64": (65, 515, (64,)),                    # N - 1 = 64: the one column of the last tile
    "65-c0": (65, 515, (0,)),
    "65-c63": (65, 515, (63,)),
    "130-c0-63-64-129": (130, 515, (0, 63, 64, 129)),
    "130-c63": (130, 515, (63,)),
    "130-c129": (130, 515, (129,)),                # N - 1 in a last tile of two columns
    "193-c70-192": (193, 400, (70, 192)),          # tiles 1 and 3
    "257-c128-256": (257, 600, (128, 256)),        # tiles 2 and 4
    "257-c63": (257, 600, (63,)),
    "513-c0": (513, 1100, (0,)),
    "513-c64": (513, 1100, (64,)),
    "513-c63-512": (513, 1100, (63, 512)),         # tiles 0 and 8: the fold regime of k_trsv_tiles behind a failed factor
}
ZERO_LAMBDA = 1e-10                                # the first lambda of the reference's schedule (dogleg.c:806-815)


def first_bad_pivot(zero):
    """the pivot word k_potrf_tiles should leave at lambda = 0: 1 + the first zero column"""
    return 1 + min(zero)


# dogleg_optimize_dense2 on such problems (the callback of test_dense_shapes_gpu.zero_cb, nonlin 0.2, p0 = 0,
# max_iterations 5): name: the (lambda, step type) of every trial the ORACLE makes -- recorded from a run of the oracle,
# asserted in test_dense_shapes_cpu.py.  "small": trustregion0 = ZERO_SMALL_TRUSTREGION, so that Cauchy steps to the
# edge (type 0) and interpolated steps (type 2) occur behind the failed pivot
ZERO_SOLVES = ("65-c64", "130-c0-63-64-129", "193-c70-192", "257-c128-256", "513-c63-512")
ZERO_SMALL_TRUSTREGION = 0.05
ZERO_MAX_ITERATIONS = 5
ZERO_TRIALS = {name: [(1e-10, 1)] * 5 for name in ZERO_SOLVES}          # the first factorisation fails; Gauss-Newton steps
ZERO_TRIALS_SMALL = {
    "65-c64": [(0.0, 0)] * 3 + [(1e-10, 1)] * 2,
    "130-c0-63-64-129": [(0.0, 0)] * 3 + [(1e-10, 1)] * 2,
    "193-c70-192": [(0.0, 0)] * 3 + [(1e-10, 2), (1e-10, 1)],
    "257-c128-256": [(0.0, 0)] * 3 + [(1e-10, 2), (1e-10, 1)],
    "513-c63-512": [(0.0, 0)] * 3 + [(1e-10, 2), (1e-10, 1)],
}

# several failures in a row, products form: J'J = A'A with column k of A zero, then entry (k, k) = NEG_PIVOT:
# lambda = 0, 1e-10, 1e-9, 1e-8 all leave a negative pivot; 1e-7 is the first that factorises.  (N, k)
NEG_PIVOT = -3e-8
NEG_CASES = ((65, 63), (65, 64), (130, 63), (130, 129))
NEG_M = {65: 515, 130: 515}
NEG_LAMBDA_COLUMN = [1e-7, 1e-7]                   # the oracle's: two trials, both at the lambda that sticks


def dense_cb(J0, xs, nonlin=0.2):
    """x = r + nonlin sin r, r = J0 p - xs; J = diag(1 + nonlin cos r) J0: a zero column of J0 stays exactly zero
    (the callback of tests/test_edge_cases_gpu.py)"""
    M, N = J0.shape

    @CB_DENSE
    def cb(p, x, J, cookie):
        pv = np.ctypeslib.as_array(p, shape=(N,)).copy()
        r = J0 @ pv - xs
        np.ctypeslib.as_array(x, shape=(M,))[:] = r + nonlin * np.sin(r)
        np.ctypeslib.as_array(J, shape=(M * N,))[:] = (J0 * (1.0 + nonlin * np.cos(r))[:, None]).ravel()
    return cb


def zero_solve(name):
    """(J0, xs, p0) of the solve on ZERO_CASES[name]"""
    N, M, zero = ZERO_CASES[name]
    x, J, p = inputs(N, M, zero)
    return J, x, np.zeros(N)


def neg_products(N, k, packed):
    """(callback, H): x = A p - xs with column k of A zero; norm2x = |x|^2, Jtx = A'x, JtJ = H = fl(A'A) with
    H[k, k] = NEG_PIVOT, whatever p -- packed upper or full"""
    x, A, p = inputs(N, NEG_M[N], (k,))
    H = A.T @ A
    H = 0.5 * (H + H.T)
    H[k, k] = NEG_PIVOT
    out = H[np.triu_indices(N)].copy() if packed else H.copy()

    @CB_PRODUCTS
    def cb(p, norm2x, Jtx, JtJ, cookie):
        r = A @ np.ctypeslib.as_array(p, shape=(N,)) - x
        norm2x[0] = float(r @ r)
        np.ctypeslib.as_array(Jtx, shape=(N,))[:] = A.T @ r
        np.ctypeslib.as_array(JtJ, shape=(out.size,))[:] = out.ravel()
    return cb, H
