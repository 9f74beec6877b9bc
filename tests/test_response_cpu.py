"""CPU: the numpy restatement of the mean-response surfaces (tests/_response_ref.py) -- the two
rules that place the integration columns, the closed form through alpha = A^-1 w against the
oracle's predict-and-average on the reference's own point sets, and the integration design.
"""
import os

import numpy as np
import pytest
import scipy.linalg as sla

import _response_ref as ref
from oracle import gp_ref


def test_cyclic_rule_by_hand():
    """d = 3, free dimension 1: column 0 -> dimension 2, column 1 -> dimension 0."""
    assert ref.int_dims(1, ref.CYCLIC, 3) == [2, 0]
    Xint = np.array([[0.1, 0.2], [0.3, 0.4]])
    P = ref.points(1, ref.CYCLIC, 0.75, None, Xint, 3)
    np.testing.assert_array_equal(P, [[0.2, 0.75, 0.1], [0.4, 0.75, 0.3]])
    # the reference's own statement of it (dnums = (arange + d_index) mod d)
    dnums = np.mod(np.arange(3) + 1, 3)
    want = np.zeros((2, 3))
    want[:, 1] = 0.75
    want[:, dnums[1:]] = Xint
    np.testing.assert_array_equal(P, want)
    assert ref.int_dims(0, ref.CYCLIC, 1) == []
    np.testing.assert_array_equal(ref.points(0, ref.CYCLIC, 0.5, None, None, 1), [[0.5]])


def test_ascending_rule_with_a_reversed_pair():
    """d = 4, pair (3, 1): the columns go to dimensions 0 and 2; x_3 = t1, x_1 = t2."""
    assert ref.int_dims((3, 1), ref.ASCENDING, 4) == [0, 2]
    Xint = np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])
    P = ref.points((3, 1), ref.ASCENDING, 0.25, 0.875, Xint, 4)
    np.testing.assert_array_equal(P, [[0.1, 0.875, 0.2, 0.25], [0.3, 0.875, 0.4, 0.25],
                                      [0.5, 0.875, 0.6, 0.25]])
    assert ref.int_dims(2, ref.ASCENDING, 4) == [0, 1, 3]
    assert ref.int_dims((0, 1), ref.ASCENDING, 2) == []


@pytest.fixture(scope="module")
def design(golden_dir):
    return np.loadtxt(os.path.join(golden_dir, "synthetic_train_standard.csv"), delimiter=",",
                      skiprows=1, comments=None)


@pytest.mark.parametrize("n,d,effect,order,T,I,delta", [
    (17, 1, 0, "cyclic", 11, 0, 1e-2),
    (64, 2, (1, 0), "ascending", 5, 0, 1e-4),
    (128, 3, 1, "cyclic", 11, 20, 1e-4),
    (128, 3, (2, 0), "ascending", 4, 10, 1e-4),
    (512, 8, 5, "cyclic", 11, 20, 1e-6),
    (512, 8, (6, 2), "ascending", 11, 10, 1e-6),
    (300, 8, 3, "ascending", 11, 20, 1e-6),
])
def test_closed_form_matches_predict_and_average(design, n, d, effect, order, T, I, delta):
    from gladsgp_amd import response
    X = design[:n, :d]
    rng = np.random.default_rng([n, d])
    beta = rng.uniform(0.5, 5.0, d)
    s = 1.3
    w = np.sin(2 * np.pi * X @ rng.uniform(0, 1, d)) + 0.1 * np.sum(X * X, axis=1)
    nfree = len(ref.free_dims(effect))
    Xint = response.integration_design(d - nfree, I) if d > nfree else None
    t = np.linspace(0, 1, T)
    t2 = t[::-1].copy() if nfree == 2 else None
    L = np.linalg.cholesky(gp_ref.gram_ardse(X, beta, s, delta))
    alpha = sla.cho_solve((L, True), w)
    got = ref.direct(X, alpha, beta, s, effect, order, t, t2, Xint)
    want = ref.predicted(X, w, beta, s, delta, effect, order, t, t2, Xint)
    assert got.shape == ((T,) if nfree == 1 else (T, T))
    err = np.max(np.abs(got - want))
    print(f"n={n} d={d} effect={effect} err {err:.3e}")
    assert err <= 1e-8 * max(1.0, np.max(np.abs(want)))
    # alpha the way the library forms it, L^-T (L^-1 w) from the explicit inverse
    Linv = sla.solve_triangular(L, np.eye(n), lower=True)
    got2 = ref.direct(X, Linv.T @ (Linv @ w), beta, s, effect, order, t, t2, Xint)
    err2 = np.max(np.abs(got2 - want))
    print(f"n={n} d={d} effect={effect} err through L^-1 {err2:.3e}")
    assert err2 <= 1e-8 * max(1.0, np.max(np.abs(want)))
    assert (np.abs(got) <= ref.bound(X, alpha, beta, s, effect, order, t, t2, Xint) *
            (1 + 1e-12)).all()


def test_integration_design_is_the_reference_lhs(golden_dir):
    """The sampler call of mean_response.py:86-88, pinned by the design tests/test_oracle.py
    regenerates with it."""
    from gladsgp_amd import response
    Xt = np.loadtxt(os.path.join(golden_dir, "synthetic_test_standard.csv"), delimiter=",",
                    skiprows=1, comments=None)
    np.testing.assert_allclose(response.integration_design(8, 100, seed=42186), Xt, atol=6e-7)
    D = response.integration_design(7, 20)
    assert D.shape == (20, 7) and (D >= 0).all() and (D <= 1).all()
    np.testing.assert_array_equal(D, response.integration_design(7, 20, seed=20240418))
    # one point per stratum in every column
    assert (np.sort(np.floor(D * 20), axis=0) == np.arange(20)[:, None]).all()
    assert response.integration_design(0, 5).shape == (5, 0)
