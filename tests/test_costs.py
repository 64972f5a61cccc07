"""The host arithmetic of the ProbsToCosts job (cluster_tools_amd/costs/probs_to_costs.py): the
cost formula, the weighting by edge size, invert_inputs and each node-label mode on a six-edge
table.  CPU only."""
import math

import numpy as np
import pytest

from cluster_tools_amd.costs import probs_to_costs as P2C

DEFAULTS = P2C.ProbsToCostsLocal.default_task_config()

# six edges over five nodes; nodes 1 and 2 are labelled
UV = np.array([[0, 1], [1, 2], [2, 3], [3, 4], [0, 4], [1, 3]], dtype=np.uint64)
PROBS = np.array([.1, .2, .5, .7, .9, .3])
LABELS = np.array([0, 1, 1, 0, 0], dtype=np.uint64)


def _formula(p, beta):
    q = (.999 - .001) * p + .001
    return math.log((1. - q) / q) + math.log((1. - beta) / beta)


@pytest.mark.parametrize('beta', [.5, .25])
def test_cost_formula(beta):
    got = P2C.probabilities_to_costs(np.array([0., .5, 1.]), beta=beta)
    want = [_formula(p, beta) for p in (0., .5, 1.)]
    np.testing.assert_allclose(got, want, rtol=1e-15, atol=1e-15)
    shift = math.log((1. - beta) / beta)
    # p = 0 is attractive, p = 1 repulsive, symmetric about the beta shift; p = .5 is the shift alone
    assert got[0] - shift > 0 > got[2] - shift and abs(got[1] - shift) < 1e-15
    assert abs((got[0] - shift) + (got[2] - shift)) < 1e-12
    assert abs(got[0] - shift - math.log(999.)) < 1e-12


def test_defaults_and_surface():
    assert {k: DEFAULTS[k] for k in ('invert_inputs', 'transform_to_costs', 'weight_edges', 'weighting_exponent',
                                     'beta')} == {'invert_inputs': False, 'transform_to_costs': True,
                                                  'weight_edges': False, 'weighting_exponent': 1., 'beta': .5}
    assert P2C.ProbsToCostsLocal.task_name == 'probs_to_costs' and P2C.ProbsToCostsLocal.allow_retry is False
    assert P2C.ProbsToCostsLocal.label_modes == ('ignore', 'isolate', 'ignore_transition')


def test_weighting():
    sizes = np.array([1., 2., 4., 8., 8., 2.])
    plain = P2C.compute_costs(PROBS, DEFAULTS)
    np.testing.assert_array_equal(plain, P2C.probabilities_to_costs(PROBS))
    # weight_edges off: the sizes are not used
    np.testing.assert_array_equal(P2C.compute_costs(PROBS, DEFAULTS, edge_sizes=sizes), plain)
    w1 = P2C.compute_costs(PROBS, dict(DEFAULTS, weight_edges=True), edge_sizes=sizes)
    np.testing.assert_array_equal(w1, plain * (sizes / 8.))
    w2 = P2C.compute_costs(PROBS, dict(DEFAULTS, weight_edges=True, weighting_exponent=2.), edge_sizes=sizes)
    np.testing.assert_array_equal(w2, plain * (sizes / 8.) ** 2.)


def test_invert_inputs_and_no_transform():
    inv = P2C.compute_costs(PROBS, dict(DEFAULTS, invert_inputs=True))
    np.testing.assert_array_equal(inv, P2C.probabilities_to_costs(1. - PROBS))
    np.testing.assert_allclose(inv, -P2C.probabilities_to_costs(PROBS), rtol=1e-12)
    raw = P2C.compute_costs(PROBS, dict(DEFAULTS, transform_to_costs=False, invert_inputs=True))
    np.testing.assert_array_equal(raw, 1. - PROBS)


def _modes(mode):
    plain = P2C.probabilities_to_costs(PROBS)
    rep, att = 5 * plain.min(), 5 * plain.max()
    assert rep < 0 < att
    got = P2C.compute_costs(PROBS, DEFAULTS, uv_ids=UV, node_labels={mode: LABELS})
    return plain, rep, att, got


def test_mode_ignore():
    """every edge touching node 1 or 2 is maximally repulsive (np.isin: the reference's np.isn)"""
    plain, rep, att, got = _modes('ignore')
    touched = np.array([True, True, True, False, False, True])
    np.testing.assert_array_equal(got[touched], rep)
    np.testing.assert_array_equal(got[~touched], plain[~touched])


def test_mode_isolate():
    plain, rep, att, got = _modes('isolate')
    np.testing.assert_array_equal(got, [rep, att, rep, plain[3], plain[4], rep])


def test_mode_ignore_transition():
    plain, rep, att, got = _modes('ignore_transition')
    labels = np.array([0, 1, 2, 2, 0], dtype=np.uint64)
    got = P2C.compute_costs(PROBS, DEFAULTS, uv_ids=UV, node_labels={'ignore_transition': labels})
    np.testing.assert_array_equal(got, [rep, rep, plain[2], rep, plain[4], rep])


def test_unknown_mode_and_short_labels():
    with pytest.raises(RuntimeError, match='Invalid label mode'):
        P2C.compute_costs(PROBS, DEFAULTS, uv_ids=UV, node_labels={'other': LABELS})
    with pytest.raises(AssertionError):
        P2C.compute_costs(PROBS, DEFAULTS, uv_ids=UV, node_labels={'ignore': LABELS[:4]})
