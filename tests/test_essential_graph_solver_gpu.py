"""k_eg_factor_solve of csrc/essential_graph.hip alone, through the real symbolic phase (aos2_debug_essential_graph_solve_device): the
block-sparse LDL^T of a symmetric matrix of 7x7 blocks in device memory and the two substitutions, against a long double dense solve.

Bound.  The kernel is the unpivoted LDL^T recurrence carried out block by block (the 7x7 diagonal blocks factored by the same
recurrence, the sums of the trailing update split by column instead of running along a row), so tests/ldlt_ref.py's condition applies
as it stands: the componentwise backward error omega = max_i |b - A x|_i / ((3 n + 1) 2^-53 (|L||D||L|^T |x|)_i) <= 1 (Higham, Theorem
10.4), with L, D from the long double factorisation.  It holds whatever the conditioning, so the lambda-only pivots of fix_scale
(1e-16 beside entries of size 1) need no bound of their own.  x itself is compared with the long double solution for the record."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldlt_ref  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 9, 17, 65, 130)
PATTERNS = ("chain", "chain_dense_rows", "arrow")


def pattern(kind, nb):
    """the lower-triangle block pairs (row, col); a pair of the chain is named twice, as duplicate edges make it"""
    pairs = [(i, i - 1) for i in range(1, nb)]
    if kind == "chain_dense_rows":
        pairs += [(r, c) for r in range(max(1, nb - 3), nb) for c in range(0, r - 1)]
    if kind == "arrow":
        pairs = [(nb - 1, c) for c in range(nb - 1)] + ([(1, 0)] if nb > 2 else [])
    if kind != "arrow" and nb > 2:
        pairs += [(2, 1)]
    return np.array(pairs, np.int32).reshape(-1, 2)


def system(kind, nb, fix_scale=False, seed=0):
    """J^T J of random 7x7 Jacobians over the pattern's pairs plus a small multiple of I -> (pairs, val, diag, b, the dense matrix)"""
    rng = np.random.default_rng([seed, nb, PATTERNS.index(kind), int(fix_scale)])
    pairs = pattern(kind, nb)
    diag = np.zeros((nb, 7, 7))
    val = np.zeros((len(pairs), 7, 7))
    A = np.zeros((7 * nb, 7 * nb))
    scale = np.ones(7) if not fix_scale else np.array([1, 1, 1, 1, 1, 1, 0.0])
    for k, (r, c) in enumerate(pairs):
        Jr, Jc = rng.normal(size=(7, 7)) * scale, rng.normal(size=(7, 7)) * scale
        diag[r] += Jr.T @ Jr
        diag[c] += Jc.T @ Jc
        val[k] = Jr.T @ Jc
        A[7 * r:7 * r + 7, 7 * c:7 * c + 7] += val[k]
    diag += (np.eye(7) * scale) * 0.5
    for i in range(nb):
        A[7 * i:7 * i + 7, 7 * i:7 * i + 7] = diag[i]
    A = np.tril(A) + np.tril(A, -1).T
    b = rng.normal(size=7 * nb) * np.tile(scale, nb)
    return pairs, val, diag, b, A


@pytest.fixture(scope="module")
def handle(pkg, gpu):
    return pkg.capi.LocalBA(device=0)


@pytest.mark.parametrize("kind", PATTERNS)
@pytest.mark.parametrize("nb", SIZES)
def test_block_sparse_solve_meets_the_backward_error_bound(handle, kind, nb):
    for fix_scale, lam in ((False, 1e-3), (True, 1e-16)):
        pairs, val, diag, b, A = system(kind, nb, fix_scale)
        x, ok, l_blocks = handle.debug_essential_graph_solve(nb, pairs[:, 0], pairs[:, 1], val, diag, b, lam)
        # (at 130 blocks the factors that scale the bound are float64 ones, seconds cheaper; the residual in omega stays long double)
        ref = ldlt_ref.ldlt_solve(A + lam * np.eye(7 * nb), b, ldlt_ref.LD if nb <= 65 else np.float64)
        assert ok == 1 and ref is not None
        Lr, dr, xr = ref
        om, row = ldlt_ref.omega(A + lam * np.eye(7 * nb), b, x, Lr, dr)
        print(kind, nb, "fix_scale", fix_scale, "l_blocks", l_blocks, "omega %.3f at row %d" % (om, row), "largest |x - x_ref| %.2e" % np.abs(x - xr.astype(np.float64)).max())
        assert om <= 1.0
        if fix_scale:   # the pivot of a scale row is lambda alone; the factorisation passes through it with x = 0 there
            assert (x[6::7] == 0).all()
        n_pairs = len({(int(r), int(c)) for r, c in pairs})
        assert l_blocks >= n_pairs and (kind != "chain" or l_blocks == nb - 1)


@pytest.mark.parametrize("nb,at", [(1, 0), (9, 0), (9, 4), (17, 16), (65, 40)])
def test_an_exactly_singular_block_fails_and_leaves_x_untouched(handle, nb, at):
    """a diagonal block whose row and column 3 are zero (and nothing else in that row of the matrix): the pivot is exactly 0"""
    pairs, val, diag, b, A = system("chain", nb)
    diag[at][3, :] = 0
    diag[at][:, 3] = 0
    for k, (r, c) in enumerate(pairs):
        if r == at:
            val[k][3, :] = 0
        if c == at:
            val[k][:, 3] = 0
    x0 = np.arange(7.0 * nb) + 0.25
    x, ok, _ = handle.debug_essential_graph_solve(nb, pairs[:, 0], pairs[:, 1], val, diag, b, 0.0, x0=x0)
    assert ok == 0 and x.tobytes() == x0.tobytes()
    x, ok, _ = handle.debug_essential_graph_solve(nb, pairs[:, 0], pairs[:, 1], val, diag, b, 1e-16, x0=x0)   # lambda alone makes it a pivot
    assert ok == 1 and np.isfinite(x).all()
