"""tests/fit_torch_ref.py::fit_reference - the one autograd statement of the fit's graph - against itself: an option that
is off adds no arithmetic, so the options' neutral values give the plain step's bits.  2 rows, random maps with 3 % of the
bits set, weights synthetic(5); four evaluations in all.  (tests/test_fit_ref64.py holds it to the independent second
statement, tests/fit_ref64.py.)"""
import numpy as np
import pytest

from oracle import pyoracle
from tests.fit_torch_ref import fit_reference


@pytest.fixture(scope="module")
def case():
    from ofighters_amd.agents.policy_weights import synthetic
    _, shapes = pyoracle.policy_init(1)
    n, rs = 2, np.random.RandomState(12)
    args = (synthetic(5).astype(np.float64), shapes, (rs.uniform(size=(n, 2, 400, 400)) < 0.03).astype(np.float64),
            rs.uniform(-1, 1, (n, 8)).astype(np.float32), rs.randint(0, 2, n).astype(np.int64),
            rs.randint(0, 400, n).astype(np.int64), rs.randint(0, 400, n).astype(np.int64),
            rs.uniform(-1, 2, n).astype(np.float32), rs.uniform(-1, 2, n).astype(np.float32))
    plain = fit_reference(*args)
    assert np.abs(plain["g"]).max() > 0
    return args, plain


def test_unit_row_weights_are_the_plain_step(case):
    args, plain = case
    ones = fit_reference(*args, row_w=np.ones(2))
    assert ones["l1"] == plain["l1"] and ones["l2"] == plain["l2"] and np.array_equal(ones["g"], plain["g"])


def test_huber_above_every_error_is_half_the_plain_step(case):
    """0.5 e^2 in place of e^2: halving is exact in binary floating point, so the comparison is =="""
    args, plain = case
    delta = 1e30
    assert delta > np.abs(plain["e"]).max()
    half = fit_reference(*args, huber_delta=delta)
    assert half["l1"] == 0.5 * plain["l1"] and half["l2"] == 0.5 * plain["l2"]
    assert (half["g"] == 0.5 * plain["g"]).all()


def test_forward_only(case):
    args, plain = case
    fwd = fit_reference(*args, backward=False)
    assert fwd["g"] is None and np.array_equal(fwd["e"], plain["e"])


def test_dense_targets_refuse_row_weights(case):
    args, _ = case
    dense = (np.zeros((2, 2)), np.zeros((2, 400, 400)))
    with pytest.raises(ValueError):
        fit_reference(*args[:4], dense=dense, row_w=np.ones(2))
