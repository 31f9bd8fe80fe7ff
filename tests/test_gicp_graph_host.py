"""The dense numpy LM of tests/gicp_lm_ref.py (Omega re-evaluated from the covariances at every linearisation and every
trial) on its own, without a GPU: the conditions under which the GPU comparison of tests/test_gicp_graph.py is fair and
decisive.  Every case decides at |rho| >= 0.1; the same LM run with Omega FROZEN at the initial poses differs from it in
chi2 by more than 100 x the tolerance of some iteration, so an implementation that does not follow the poses cannot pass;
the measured self-sensitivities are printed."""
import functools

import numpy as np
import pytest

import gicp_lm_ref as G
import icp_lm_ref


@functools.lru_cache(maxsize=None)
def reference(name, frozen=False):
    recipe, niter = G.CASES[name]
    return G.reference_runs(*recipe(), niter, frozen=frozen)


@pytest.mark.parametrize("name", ["scan_to_map", "multi_scan", "mixed", "iso"])
def test_every_decision_is_clear_and_the_sensitivity_is_small(name):
    tr, pose, lm, sens, est = reference(name)
    print("reference %s: self-sensitivity %.3g (chi2), %.3g (estimates); trials %s; chi2 %s" %
          (name, max(sens), est, [t["trials"] for t in tr], ["%.9g" % t["chi2"] for t in tr]))
    assert len(tr) == G.CASES[name][1]
    assert all(abs(t["rho"]) >= 0.1 for t in tr), [t["rho"] for t in tr]
    assert max(sens) < 1e-12 and tr[-1]["chi2"] < tr[0]["chi2"]


@pytest.mark.parametrize("name", ["scan_to_map", "multi_scan"])
def test_a_frozen_omega_cannot_pass(name):
    tr, _, _, sens, est = reference(name)
    frozen = reference(name, True)[0]
    tol, _ = icp_lm_ref.tolerances(sens, est)
    ratio = [abs(a["chi2"] - b["chi2"]) / b["chi2"] / t for a, b, t in zip(frozen, tr, tol)]
    print(name, "chi2 with Omega frozen at the initial poses differs by (x tolerance):", ["%.3g" % r for r in ratio])
    assert max(ratio) > 100


def test_the_start_of_scan_to_map_is_10_to_20_degrees_away():
    d = G.scan_to_map_case()[0]
    q0, q1 = np.asarray(d["pose"])[:, :4], np.asarray(d["pose_gt"])[:, :4]
    ang = np.rad2deg(2 * np.arccos(np.clip(np.abs((q0 * q1).sum(1)), 0, 1)))
    free = np.asarray(d["pose_fixed"]) == 0
    assert np.all((ang[free] > 9.99) & (ang[free] < 20.01)) and np.all(ang[~free] == 0)
