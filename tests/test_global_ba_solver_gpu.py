"""k_gba_factor_solve of csrc/global_ba.hip alone, through the real symbolic phase (aos2_debug_global_ba_solve_device): block_ldlt.h's
block-sparse LDL^T with 6x6 blocks in device memory and the two substitutions, against a long double dense solve.

Bound: the one tests/test_essential_graph_solver_gpu.py uses for the 7x7 instance of the same code.  The kernel is the unpivoted LDL^T
recurrence carried out block by block, so tests/ldlt_ref.py's condition applies as it stands: the componentwise backward error
omega = max_i |b - A x|_i / ((3 n + 1) 2^-53 (|L||D||L|^T |x|)_i) <= 1 (Higham, Theorem 10.4), with L, D from the reference
factorisation.  It holds whatever the conditioning.  x itself is compared with the reference solution for the record."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldlt_ref  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 17, 65, 160)
PATTERNS = ("band", "arrow", "random")


def pattern(kind, nb, rng):
    """the lower-triangle block pairs (row, col); one pair is named twice, as two landmarks shared by the same keyframes make it"""
    if kind == "band":
        pairs = [(r, c) for r in range(nb) for c in range(max(0, r - 3), r)]
    elif kind == "arrow":   # the last column dense, and a chain
        pairs = [(nb - 1, c) for c in range(nb - 1)] + [(r, r - 1) for r in range(1, nb - 1)]
    else:
        pairs = [(r, c) for r in range(nb) for c in range(r) if rng.random() < min(1.0, 4.0 / nb)]
    if nb > 2:
        pairs += [(2, 1)]
    return np.array(pairs, np.int32).reshape(-1, 2)


def system(kind, nb, seed=0):
    """J^T J of random 6x6 Jacobians over the pattern's pairs plus a small multiple of I -> (pairs, val, diag, b, the dense matrix)"""
    rng = np.random.default_rng([seed, nb, PATTERNS.index(kind)])
    pairs = pattern(kind, nb, rng)
    diag = np.zeros((nb, 6, 6))
    val = np.zeros((len(pairs), 6, 6))
    A = np.zeros((6 * nb, 6 * nb))
    for k, (r, c) in enumerate(pairs):
        Jr, Jc = rng.normal(size=(6, 6)), rng.normal(size=(6, 6))
        diag[r] += Jr.T @ Jr
        diag[c] += Jc.T @ Jc
        val[k] = Jr.T @ Jc
        A[6 * r:6 * r + 6, 6 * c:6 * c + 6] += val[k]
    diag += np.eye(6) * 0.5
    for i in range(nb):
        A[6 * i:6 * i + 6, 6 * i:6 * i + 6] = diag[i]
    A = np.tril(A) + np.tril(A, -1).T
    return pairs, val, diag, rng.normal(size=6 * nb), A


@pytest.fixture(scope="module")
def handle(pkg, gpu):
    return pkg.capi.LocalBA(device=0)


@pytest.mark.parametrize("kind", PATTERNS)
@pytest.mark.parametrize("nb", SIZES)
def test_block_sparse_solve_meets_the_backward_error_bound(handle, kind, nb):
    pairs, val, diag, b, A = system(kind, nb)
    for lam in (0.0, 1e-3):
        x, ok, l_blocks = handle.debug_global_ba_solve(nb, pairs[:, 0], pairs[:, 1], val, diag, b, lam)
        # (at 160 blocks the factors that scale the bound are float64 ones, seconds cheaper; the residual in omega stays long double)
        ref = ldlt_ref.ldlt_solve(A + lam * np.eye(6 * nb), b, ldlt_ref.LD if nb <= 65 else np.float64)
        assert ok == 1 and ref is not None
        Lr, dr, xr = ref
        om, row = ldlt_ref.omega(A + lam * np.eye(6 * nb), b, x, Lr, dr)
        print(kind, nb, "lambda", lam, "l_blocks", l_blocks, "omega %.3f at row %d" % (om, row), "largest |x - x_ref| %.2e" % np.abs(x - xr.astype(np.float64)).max())
        assert om <= 1.0
        n_pairs = len({(int(r), int(c)) for r, c in pairs})
        assert l_blocks >= n_pairs and (kind != "band" or l_blocks == n_pairs)   # a band has no fill


@pytest.mark.parametrize("nb,at", [(1, 0), (17, 0), (17, 9), (65, 64), (160, 100)])
def test_a_planted_zero_pivot_fails_and_leaves_x_untouched(handle, nb, at):
    """a diagonal block whose row and column 3 are zero (and nothing else in that row of the matrix): the pivot is exactly 0"""
    pairs, val, diag, b, A = system("band", nb)
    diag[at][3, :] = 0
    diag[at][:, 3] = 0
    for k, (r, c) in enumerate(pairs):
        if r == at:
            val[k][3, :] = 0
        if c == at:
            val[k][:, 3] = 0
    x0 = np.arange(6.0 * nb) + 0.25
    x, ok, _ = handle.debug_global_ba_solve(nb, pairs[:, 0], pairs[:, 1], val, diag, b, 0.0, x0=x0)
    assert ok == 0 and x.tobytes() == x0.tobytes()
    x, ok, _ = handle.debug_global_ba_solve(nb, pairs[:, 0], pairs[:, 1], val, diag, b, 1e-16, x0=x0)   # lambda alone makes it a pivot
    assert ok == 1 and np.isfinite(x).all()
