"""The first linearisation of an essential graph as the device forms it (aos2_debug_essential_graph_linearised_device: the call's host
phase and layout, then k_eg_perturb, k_eg_linearise, k_eg_assemble, k_eg_begin) on the inputs of tests/essential_graph_cases.py: edges
in both orientations between free vertices, a free pair named twice, the fixed vertex first, last and in the middle, edge and vertex
counts on both sides of the 256 threads of a workgroup.

H and b: the build has -ffp-contract=off and no fast-math, every entry is a sum in a fixed order that starts from 0, and a product of
two doubles is the same number on the device and in numpy, so K.replay on the DEVICE's J and E -- a plain walk over the edges that
knows v0, v1 and `fixed` only -- must give the device's H and b bit for bit.  A wrong list, a term in the wrong slot, the wrong one of
J0^T J1 / J1^T J0 or a sum in another order all show.
E against R.residuals within the bound of test_header_residual_agrees_with_the_restatement (128 DBL_EPSILON M); J against the closed
form within the bound of test_central_difference_jacobian_agrees_with_the_closed_form (100 M DBL_EPSILON / delta); chi2 against the
long double sum of the device's own residuals within (ne + 8) 2^-53 chi2: ne additions and the 7 products and 6 additions of one
residual's square, each half an ulp of a partial sum that is at most chi2.
What was measured is written to profiles/essential_graph_taps.txt."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essential_graph_cases as K  # noqa: E402
import essential_graph_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def handle(pkg, gpu):
    return pkg.capi.LocalBA(device=0)


@pytest.mark.parametrize("name", list(K.cases()))
def test_linearisation_is_the_replay_of_its_own_jacobians_bit_for_bit(handle, name):
    P = K.cases()[name]
    est = np.asarray(P["Scw"], np.float64)
    ne, fixed, fix = len(P["v0"]), P["fixed"], bool(P["fix_scale"])
    got = handle.debug_essential_graph_linearised(P)
    J, E, H, b = got["J"], got["E"], got["H"], got["b"]

    # the Jacobian of a fixed side is never written; every other one is
    side_fixed = np.stack([P["v0"] == fixed, P["v1"] == fixed], axis=1)
    assert side_fixed.any() and (J[side_fixed].view(np.uint8) == SENTINEL).all()
    assert np.isfinite(J[~side_fixed]).all() and not (J[~side_fixed].view(np.uint8).reshape(-1, 49 * 8) == SENTINEL).all(axis=1).any()

    # H and b: the replay, bit for bit
    Hr, br = K.replay(P, J, E)
    print(name, "edges", ne, "free pairs", K.free_pairs(P), "l_blocks", got["l_blocks"], "largest |H - replay| %.3g, |b - replay| %.3g" %
          (np.abs(H - Hr).max(), np.abs(b - br).max()))
    assert H.tobytes() == Hr.tobytes() and b.tobytes() == br.tobytes()
    assert (H[~K.pattern(P)] == 0).all() and np.array_equal(H, H.T)
    if fix:
        assert (H[6::7, :] == 0).all() and (H[:, 6::7] == 0).all() and (b[6::7] == 0).all()
    if min(K.free_pairs(P)) >= 1:   # (the replay can tell: it is not blind to what these inputs add)
        assert K.replay(P, J, E, mutant="kind3")[0].tobytes() != H.tobytes()

    # E, J, chi2
    b_E = K.residual_bound(P, est)
    r_E = np.abs(E - R.residuals(P["Sji"], est, P["v0"], P["v1"])).max() / b_E
    closed, b_J, emax = K.closed_form(P, est)
    cols = 6 if fix else 7
    dJ = np.abs(np.where(side_fixed[:, :, None, None], closed, J) - closed)[..., :cols]
    r_J = (dJ.max(axis=(1, 2, 3)) / b_J).max()
    if fix:
        assert (J[~side_fixed][..., 6] == 0).all()
    chi_ld = float((E.astype(np.longdouble) ** 2).sum())
    b_chi = (ne + 8) * 2.0 ** -53 * chi_ld
    r_chi = abs(got["chi2"] - chi_ld) / b_chi if b_chi else float(got["chi2"] != chi_ld)
    print("   difference / bound: E %.3g, J %.3g, chi2 %.3g; largest |e| %.3f" % (r_E, r_J, r_chi, emax))
    K.record("linearised " + name, "ne %d nf %d fixed %d fix_scale %d: H and b equal the replay; E %.3g J %.3g chi2 %.3g" %
             (ne, len(est) - 1, fixed, fix, r_E, r_J, r_chi))
    assert r_E <= 1 and r_J <= 1 and r_chi <= 1
    assert got["chi2_initial"] == got["chi2"]

    # the same symbolic phase as the full call
    assert got["l_blocks"] == handle.optimize_essential_graph([dict(P, iterations=1)])[0]["l_blocks"]
