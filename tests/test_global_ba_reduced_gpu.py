"""The reduced camera system of one linearisation as the device assembles it (aos2_debug_global_ba_reduced_device: k_gba_linearise,
k_gba_sums, k_gba_landmarks, k_gba_assemble) against the dense matrix of tests/global_ba_ref.py.

Bound, per entry, derived: an entry is a sum of n_terms products -- the edges' parts of Hpp (or b), lambda, and for every pair of
edges of a landmark the three products of (B_i Dinv) B_j^T -- taken in the reference's order; a sum of n terms carried out in any
order differs from another by at most 2 (n - 1) 2^-53 sum |terms|, and the terms themselves (the same lines evaluated in float64 on
both sides: + - * / and one 3x3 inverse by cofactors) by a rounding each.  Allowed: 4 n_terms 2^-53 sum |terms|, with n_terms and
sum |terms| from the reference.  An entry outside the pattern has no term and must be exactly zero."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_ba_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle(pkg, gpu):
    return pkg.capi.LocalBA(device=0)


@pytest.mark.parametrize("robust,huber", [(False, R.HUBER_GBA), (True, R.HUBER_LOCAL_BA)])
@pytest.mark.parametrize("name", ["init", "pair", "mixed", "loop", "past_lba"])
def test_reduced_system_agrees_with_the_dense_reference_entry_by_entry(handle, name, robust, huber):
    prob = R.problem(name)
    G = R.Graph(prob, robust, huber)
    S = G.build()
    lam0 = 1e-5 * max(np.abs(S["Hpp"][:, range(6), range(6)]).max(), np.abs(S["Hll"][:, range(3), range(3)]).max())
    for lam in (lam0, 64 * lam0):
        want = G.reduce(S, lam)
        got_S, got_bs, h_blocks = handle.debug_global_ba_reduced(prob, lam, G.np_, robust, huber)
        bound_S = 4 * want["n_S"] * 2.0 ** -53 * want["abs_S"]
        bound_b = 4 * want["n_bs"] * 2.0 ** -53 * want["abs_bs"]
        dS, db = np.abs(got_S - want["S"]), np.abs(got_bs - want["bs"])
        inside = want["n_S"] > 0
        print(name, "robust", robust, "lambda %.3g" % lam, "largest |S - ref| / bound %.3g, |bs - ref| / bound %.3g" %
              ((dS[inside] / bound_S[inside]).max(), (db / bound_b).max()), "h_blocks", h_blocks)
        assert h_blocks == G.h_blocks()
        assert (dS <= bound_S).all() and (db <= bound_b).all()
        assert (got_S[~inside] == 0).all() and np.array_equal(got_S, got_S.T)
