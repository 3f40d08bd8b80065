"""Actor-side initial priorities, the CPU side: the numpy restatement against a case worked out by hand, and the
argument checks / fingerprint of DeviceTrainer(actor_priorities=...)."""
import numpy as np
import pytest

from tests.actor_priority_oracle import ArenaOracle, td_errors

NAN = float("nan")


def test_oracle_reproduces_a_hand_computed_case():
    """alpha = 0.5, eps = 0.25, gamma = 0.5: every number below is exact in float32 and every mass a square root.
    step 1  ships 0 and 1 play for the first time: no row; prev_q <- (1, 0.5), (2, 0.25)
    step 2  ship 0: reward 1, alive, v_act 2, v_ptr 1: y = (2, 1.5), e = (-1, -1), p = 2.25, m = 1.5
            ship 1: reward 3, DONE (its v_* are NaN and must not be read): y = (3, 3), e = (-1, -2.75), p = 4, m = 2
            mmax: 1 -> 2
    step 3  ship 0 alone (ship 1 is latched): v_ptr is NaN -> the row takes mmax = 2 as read before the step; mmax stays"""
    o = ArenaOracle(2, 8, 0.5, 0.25, 0.5)
    o.capture_valued([0, 0], [0, 0], [False, False], [True, True], [1.0, 2.0], [0.5, 0.25], [9.0, 9.0], [9.0, 9.0])
    assert list(o.mass) == [] and o.mmax == 1.0
    assert o.prev_q.tolist() == [[1.0, 0.5], [2.0, 0.25]]
    o.capture_valued([1, 3], [0, 1], [True, True], [True, True], [4.0, 5.0], [6.0, 7.0], [2.0, NAN], [1.0, NAN])
    assert list(o.mass) == [1.5, 2.0] and o.mmax == 2.0 and o.fallbacks == 0
    o.capture_valued([0, 0], [0, 1], [True, False], [True, False], [0.0, -1.0], [0.0, -1.0], [1.0, 1.0], [NAN, 1.0])
    assert list(o.mass) == [1.5, 2.0, 2.0] and o.mmax == 2.0 and o.fallbacks == 1
    assert o.prev_q.tolist() == [[0.0, 0.0], [5.0, 7.0]]          # the latched ship's values are not replaced
    # a raise by a later row, after a fallback: e = (0 - (0 + 0.5 * 8), 0 - (0 + 0.5 * 8)) = (-4, -4), p = 8.25
    o.capture_valued([0, 0], [0, 1], [True, False], [True, False], [0.0, 0.0], [0.0, 0.0], [8.0, 0.0], [8.0, 0.0])
    assert o.mass[-1] == 8.25 ** 0.5 and o.mmax == 8.25 ** 0.5
    o.capture_plain([True, False])
    assert o.mass[-1] == o.mmax and o.prev_q.tolist() == [[0.0, 0.0], [5.0, 7.0]]


def test_td_errors_round_like_the_learner():
    """The product rounds before the sum (no fused multiply-add): 0.9f * 3 = 2.7000000477 -> float32, + 1e8 -> float32."""
    f = np.float32
    e1, e2 = td_errors(7, 0, 0.1, 0.2, 3.0, 1e-3, 0.9)
    assert e1 == f(f(0.1) - f(f(7) + f(f(0.9) * f(3.0)))) and e2 == f(f(0.2) - f(f(7) + f(f(0.9) * f(1e-3))))
    assert td_errors(7, 1, 0.5, 0.25, NAN, float("inf"), 0.9) == (f(-6.5), f(-6.75))
    assert not np.isfinite(td_errors(0, 0, 0.5, 0.25, 1.0, float("inf"), 0.9)[1])


def test_the_ring_drops_the_oldest_mass():
    o = ArenaOracle(1, 2, 0.5, 0.25, 0.5)
    for k in range(4):
        o.capture_valued([k], [0], [k > 0], [True], [0.0], [0.0], [0.0], [0.0])
    assert len(o.mass) == 2 and list(o.mass) == [(2 * 2 + 0.25) ** 0.5, (2 * 3 + 0.25) ** 0.5]


@pytest.mark.parametrize("kw, word", [(dict(actor_priorities=1), "bool"),
                                      (dict(actor_priorities=True), "prioritized"),
                                      (dict(actor_priorities=True, prioritized=True, reference_quirks=True), "reference_quirks")])
def test_trainer_refuses_before_anything_is_allocated(kw, word):
    from ofighters_amd.trainer import DeviceTrainer
    with pytest.raises(ValueError, match="actor_priorities") as err:
        DeviceTrainer(None, np.zeros(4, np.float32), **kw)          # batch=None: any allocation would raise something else
    assert word in str(err.value)


class _Batch:
    replay_capacity, replay_frames = 400, 502


def _bare(**attrs):
    from ofighters_amd.trainer import DeviceTrainer
    t = DeviceTrainer.__new__(DeviceTrainer)
    t.batch = _Batch()
    t.n_floats, t.learning_rate, t.gamma, t.batch_size, t.fit_batch, t.seed = 10, 1e-4, 0.9, 8, 256, 1
    t.reference_quirks, t.prioritized = False, True
    t.per_alpha, t.per_beta, t.per_beta_steps, t.per_eps, t.n_step = 0.6, 0.4, 50_000, 1e-3, 1
    t.target_sync, t.target_tau, t.double_dqn, t.huber_delta, t.clip_norm = 0, None, False, None, None
    for k, v in attrs.items():
        setattr(t, k, v)
    return t


def test_fingerprint_carries_the_key_only_when_on():
    from ofighters_amd.trainer import DeviceTrainer, fingerprint_diff
    assert DeviceTrainer.actor_priorities is False
    off, on = _bare().fingerprint(), _bare(actor_priorities=True).fingerprint()
    assert "actor_priorities" not in off and on["actor_priorities"] is True
    assert fingerprint_diff(on, off) == ["actor_priorities"] == fingerprint_diff(off, on)
    assert {k: v for k, v in on.items() if k != "actor_priorities"} == off
