"""What tests/test_gpu_evolution_edges.py rests on, shown without a device: every forward case's scene takes the branch
it is there for, nothing saturates, the tolerance is one the numpy reference meets with a factor of ten to spare, and
one lost or doubled map cell misses it a thousandfold.  Everything here comes from the oracle alone."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import evolution_cases as ec
from tests import evolution_oracle as eo
from tests.boltzmann_oracle import philox_words

CASES = pytest.mark.parametrize("case", ec.FORWARD_CASES, ids=ec.case_id)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@CASES
def test_scene_takes_its_branch(case):
    kind, W, H, M, hidden, ticks, seed = case
    ref = ec.case_reference(case)
    head, sm, lm, alive = ref["obs"][0]
    words = W * H // 32
    total, per = 2 * words, (2 * words + 3) // 4
    q = ec.quarter_counts(sm, lm)
    at = ec.set_cells(sm, lm) // 32
    print("%s: words %d, quarters %s, %d ships flown" % (ec.case_id(case), words, q, len(ref["exact"])))
    assert sum(q) == int(sm.sum()) + int(lm.sum())
    if kind == "dense":
        # quarters 0 and 1 are the ship map (words is even here): the list fills and is gathered at least twice mid-walk
        assert words % 2 == 0 and max(q[:2]) > 2 * ec.POP_LIST
    elif kind == "odd":
        assert words % 2 == 1 and per < words < 2 * per, "the boundary is not inside quarter 1"
        assert ((at >= per) & (at < words)).any(), "no ship cell in quarter 1"
        assert ((at >= words) & (at < 2 * per)).any(), "no laser cell in quarter 1"
        assert lm.any()
    elif kind == "one":
        assert words == 1 and q == [32, 0, 0, 0] and (total, per) == (2, 1)
    else:
        assert kind == "plain"
    # there is something to compare, in arena 0 (the one the precondition is about) and beyond it, and a dead or
    # unassigned ship to leave alone
    assert 0 in {a for a, _ in ref["exact"]} and len(ref["exact"]) >= 2
    assert len(ref["exact"]) < ec.N_ARENAS * M or M == 1


def test_the_cases_hold_every_layout():
    """n1 of 1, 32, 33, 63 and 64, the two-layer net and the contract's eight layers; a dead ship that is assigned."""
    n1 = {ec.case_layers(c)[1] for c in ec.FORWARD_CASES}
    assert {1, 32, 33, 63, 64} <= n1
    depths = {len(ec.case_layers(c)) for c in ec.FORWARD_CASES}
    assert {2, 8} <= depths
    dead_assigned = 0
    for case in ec.FORWARD_CASES:
        ref = ec.case_reference(case)
        for a, (_, _, _, alive) in enumerate(ref["obs"]):
            dead_assigned += int(((ref["genome_of"][a] >= 0) & (alive == 0)).sum())
    assert dead_assigned > 0


@CASES
def test_nothing_saturates(case):
    ref = ec.case_reference(case)
    worst = 0.0
    for (a, i), _ in ref["exact"].items():
        head, sm, lm, _ = ref["obs"][a]
        z = ec.first_layer_exact(ref["layers"], ref["genomes"][ref["genome_of"][a, i]], head[i], sm, lm)
        worst = max(worst, max(abs(v) for v in z))
    print("%s: max |z| of the first layer %.2f" % (ec.case_id(case), worst))
    assert worst < 4


@CASES
def test_the_tolerance_is_earned_and_has_power(case):
    ref = ec.case_reference(case)
    layers, rtol = ref["layers"], ec.case_rtol(case)
    cells_run = layers[0] - 8
    dev, weakest = 0.0, np.inf
    for (a, i), exact in ref["exact"].items():
        head, sm, lm, _ = ref["obs"][a]
        g = ref["genomes"][ref["genome_of"][a, i]]
        dev = max(dev, ec.rel_dev(eo.forward(layers, g, head[i], sm, lm), exact))
        cells = ec.set_cells(sm, lm)
        drop = int(cells[len(cells) // 2])
        extra = next(c for c in range(drop + 1, drop + 1 + cells_run) if c % cells_run not in cells) % cells_run
        for kw in (dict(drop=drop), dict(extra=extra)):
            weakest = min(weakest, ec.rel_dev(ec.forward_exact(layers, g, head[i], sm, lm, **kw), exact))
    print("%s: numpy against exact %.3e, one cell dropped or added %.3e" % (ec.case_id(case), dev, weakest))
    assert dev <= rtol / 10, "the reference itself does not meet the tolerance with a factor of ten to spare"
    assert weakest > 1e3 * rtol, "one cell would pass unnoticed"


def test_forward_exact_is_the_oracles_forward_on_a_small_net():
    """forward_exact restates evolution_oracle.forward, and so Neural_network.feed: to rounding on random weights."""
    rs = np.random.RandomState(11)
    W, H = 8, 4
    layers = [8 + 2 * W * H, 5, 3, 4]
    g = rs.uniform(-1, 1, eo.n_elements(layers))
    sm, lm = (rs.random_sample((W, H)) < 0.3).astype(np.uint8), (rs.random_sample((W, H)) < 0.2).astype(np.uint8)
    head = rs.uniform(-3, 3, 8)
    Wl, Bl = eo.split(layers, g)
    dense = pyoracle.nn_feed(layers, Wl, Bl, np.concatenate([head, sm.ravel(), lm.ravel()]))
    np.testing.assert_allclose(ec.forward_exact(layers, g, head, sm, lm), dense, rtol=1e-14, atol=0)
    np.testing.assert_allclose(ec.forward_exact(layers, g, head, sm, lm), eo.forward(layers, g, head, sm, lm), rtol=1e-14, atol=0)


def test_quarter_counts_split():
    sm, lm = np.zeros((24, 20), np.uint8), np.zeros((24, 20), np.uint8)         # 15 words a map, per = 8
    sm.ravel()[[0, 255, 256, 479]] = 1                                          # words 0, 7 | 8, 14
    lm.ravel()[[0, 31, 32, 287, 288, 479]] = 1                                  # run words 15 | 16, 23 | 24, 29
    assert ec.quarter_counts(sm, lm) == [2, 4, 2, 2]
    sm, lm = np.ones((8, 4), np.uint8), np.zeros((8, 4), np.uint8)
    lm[0, 0] = 1
    assert ec.quarter_counts(sm, lm) == [32, 1, 0, 0]


BREED_LAYERS, BREED_SLOTS = ec.BREED_LAYERS, ec.BREED_SLOTS


def test_breed_draws_of_single_slots_equal_those_of_a_list_of_slots():
    """The GPU test of 70 000 slots checks sampled slots with eo.fresh / eo.child one slot at a time.  Those calls give
    the bits of the same draws made for a list of slots at once, and of the scalar Philox of the C oracle."""
    seed, G = 0x0E7090FF, eo.n_elements(BREED_LAYERS)
    assert G == 273
    slots = np.asarray(BREED_SLOTS, np.int64)
    e = np.arange(G, dtype=np.int64)
    for generation, stream in ((0, eo.STREAM_FRESH), (1, eo.STREAM_FRESH)):
        r = philox_words(seed, slots[:, None], e[None, :], generation, stream)
        together = 2.0 * eo.u(r[..., 0], r[..., 1]) - 1.0
        for k, p in enumerate(BREED_SLOTS):
            one = eo.fresh(BREED_LAYERS, seed, p, generation)
            assert np.array_equal(_bits(one), _bits(together[k])), "fresh, slot %d" % p
            for el in (0, 263, 264, 272):
                assert one[el] == eo.fresh_scalar(seed, p, el, generation)
    parent = eo.fresh(BREED_LAYERS, seed, 0, 0)
    r = philox_words(seed, slots[:, None], e[None, :], 1, eo.STREAM_EVOLVE)
    s = philox_words(seed, slots[:, None], e[None, :], 1, eo.STREAM_MUTATE)
    c = (2.0 * eo.u(r[..., 0], r[..., 1]) - 1.0) * 0.05
    w = np.multiply(c, parent[None, :]) + parent[None, :]
    w = np.where(eo.u(r[..., 2], r[..., 3]) < 0.05, 2.0 * eo.u(s[..., 0], s[..., 1]) - 1.0, w)
    mutated = 0
    for k, p in enumerate(BREED_SLOTS):
        one = eo.child(parent, seed, p, 1, 0.05, 0.05)
        assert np.array_equal(_bits(one), _bits(w[k])), "child, slot %d" % p
        mutated += int((eo.selector(BREED_LAYERS, seed, p, 1) < 0.05).sum())
    assert mutated > 0
    # a population as a list, through eo.breed: the same slots one at a time
    P = 12
    old = [eo.fresh(BREED_LAYERS, seed, p, 0) for p in range(P)]
    plan = np.array([0] * (P - 1) + [-1], np.int32)
    new = eo.breed(old, plan, 0.05, 0.05, seed, 1, BREED_LAYERS)
    assert np.array_equal(_bits(new[0]), _bits(old[0]))
    assert np.array_equal(_bits(new[P - 1]), _bits(eo.fresh(BREED_LAYERS, seed, P - 1, 1)))
    for p in range(1, P - 1):
        assert np.array_equal(_bits(new[p]), _bits(eo.child(old[0], seed, p, 1, 0.05, 0.05)))
