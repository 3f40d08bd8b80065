"""The scenarios of tests/step_constant_cases.py are what they claim to be - on the CPU, from the oracle alone.  The
GPU tests (tests/test_gpu_step_constants.py) then hold the kernels to the oracle on the very same scenarios."""
import math

import numpy as np
import pytest

from oracle import pyoracle
from tests import step_constant_cases as sc


def test_constant_sets_leave_no_default():
    d = pyoracle.default_cfg()
    for tag in sc.TAG_NAMES:
        k = sc.constants(tag)
        assert sc.HIT_RADIUS[tag] == k["ship_radius"] + k["laser_radius"]
        assert (k["width"] * k["height"]) % 32 == 0
        for f in ("reward_death", "reward_kill", "reward_aim", "reward_trajectory", "ship_radius", "ship_speed",
                  "laser_speed", "width", "height"):
            assert k[f] != getattr(d, f), (tag, f)
    assert {sc.TAGS[t]["laser_radius"] for t in sc.TAG_NAMES} == {1, 2, 3}
    # every reward decodes in one way only
    sums = {}
    for kills in range(0, 12):
        for s, rules in sc._SUBSETS.items():
            assert sums.setdefault(sc.KILL * kills + s, (kills,) + rules) == (kills,) + rules
    assert len(sc._SUBSETS) == 8 and len({s % sc.KILL for s in sc._SUBSETS}) == 8
    assert sc.decode_reward(2 * sc.KILL + sc.DEATH + sc.TRAJ) == (2, 1, 0, 1)
    from ofighters_amd import _native as nat          # the bots' numbering the oracle is given
    assert all(nat.BEHAVIOURS[name] == v for name, v in sc.BOT.items())


@pytest.mark.parametrize("tag", sc.TAG_NAMES)
def test_hit_threshold(tag):
    """T computed here with math.sqrt and math.nextafter: the largest double whose root is <= R.  The offsets the
    crafted cases use land on T and on the double after it, in the kernel's own arithmetic ddx*ddx + ddy*ddy."""
    R = sc.HIT_RADIUS[tag]
    T = sc.hit_threshold(R)
    assert math.sqrt(T) <= R < math.sqrt(math.nextafter(T, math.inf))
    # written down: one ulp above R*R for R = 5, 2 and 43 (so R*R is NOT the threshold), R*R itself for 13 and 25
    assert (T - R * R) / math.ulp(float(R * R)) == {5: 1.0, 13: 0.0, 25: 0.0, 2: 1.0, 43: 1.0}[R]
    x_hit, x_miss = sc.threshold_offsets(R)
    assert x_hit == {5: 2.0 ** -24, 13: 0.0, 25: 0.0, 2: 2.0 ** -25, 43: 2.0 ** -21}[R]
    d2_hit, d2_miss = x_hit * x_hit + float(R) * float(R), x_miss * x_miss + float(R) * float(R)
    assert d2_hit == T and d2_miss == math.nextafter(T, math.inf)
    assert math.sqrt(d2_hit) <= R < math.sqrt(d2_miss)
    if T > R * R:
        assert d2_hit > R * R
    a, b = sc.TRIPLE[R]
    assert a * a + b * b == R * R and a * a + (b + 1) * (b + 1) > R * R
    r = sc.TAGS[tag]["ship_radius"]
    if r in sc.AIM_TRIPLE:
        a, b = sc.AIM_TRIPLE[r]
        assert a * a + b * b == r * r and a > 0
    else:
        assert not [(a, b) for a in range(1, r) for b in range(1, r) if a * a + b * b == r * r]


@pytest.mark.parametrize("tag", sc.TAG_NAMES)
def test_rollout_contains_its_events(tag):
    roll = sc.OracleRollout(tag)
    assert len(set(sc.BEHAVIOURS)) == roll.M == 6 and roll.N % 4 != 0
    restarts = 0
    for _ in range(sc.ROLLOUT["ticks"]):
        if roll.restart_due():
            roll.restart()
            restarts += 1
        roll.step(roll.actions())
    assert restarts == 1 and roll.t == 60 and roll.time == 35 and sum(sc.ROLLOUT["spans"]) == 60
    assert sum(sc.ROLLOUT["spans"][:2]) < sc.ROLLOUT["restart_after"]      # the restart falls between single calls
    assert roll.events >= sc.ROLLOUT_EVENTS[tag], (tag, sorted(roll.events))
    assert {"kill", "laser_hit"} <= sc.ROLLOUT_EVENTS[tag]
    if sc.TAGS[tag]["laser_speed"] == 0:
        assert "laser_out" not in sc.ROLLOUT_EVENTS[tag]


def _run(tag, case):
    o = sc.plant(tag, case)
    states = [sc.state(o)]
    for acts in case["actions"]:
        o.step(np.array(acts, np.int32))
        states.append(sc.state(o))
    return o, states


@pytest.mark.parametrize("tag", sc.TAG_NAMES)
def test_crafted_cases_on_the_oracle(tag):
    cases = sc.crafted_cases(tag)
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names) and {c["M"] for c in cases} == {2, 3}
    for c in cases:
        assert c["expect"], c["name"]
        o, states = _run(tag, c)
        # the planted start is what the case says
        assert [(int(x), int(y)) for x, y in zip(states[0]["x"], states[0]["y"])] == [s[:2] for s in c["ships"]]
        assert list(states[0]["lx"]) == [l[0] for l in c["lasers"]] and states[0]["n_lasers"] == len(c["lasers"])
        for step in (1, 2):
            sc.check_expectation(c, step, states[step])
    by = {c["name"]: c for c in cases}
    k = sc.constants(tag)
    cfg = sc.oracle_cfg(tag, 2)
    W, H, r, R, ss, ls = k["width"], k["height"], k["ship_radius"], sc.HIT_RADIUS[tag], k["ship_speed"], k["laser_speed"]
    # hit cases: the squared distances, in the arithmetic of the collide test, sit where the case says
    T = sc.hit_threshold(R)
    for name in ("hit_integer", "hit_threshold"):
        (mx, my), (hx, hy) = [l[:2] for l in by[name]["lasers"]]
        assert hx * hx + hy * hy <= T < mx * mx + my * my, name
    hx, hy = by["hit_threshold"]["lasers"][1][:2]
    assert hx * hx + hy * hy == T
    lx, ly = by["multikill"]["lasers"][0][:2]
    for sx, sy in [s[:2] for s in by["multikill"]["ships"][:2]]:
        assert (lx - sx) ** 2 + (ly - sy) ** 2 == R * R
    # aim cases: exactly ship_radius, and one past it
    for name, d2 in (("aim_at_r", r * r), ("aim_past_r", (r + 1) * (r + 1))):
        c = by[name]
        px, py = c["actions"][0][0][3:]
        ex, ey = c["ships"][1][:2]
        assert (px - ex) ** 2 + (py - ey) ** 2 == d2
        assert pyoracle.enemy_aimed(cfg, px, py, ex, ey) == (name == "aim_at_r")
    # hit-box cases: d2 == inR^2 and inR^2 + 1
    for name, d2 in (("hitbox_on", R * R), ("hitbox_past", R * R + 1)):
        c = by[name]
        px, py = c["actions"][0][0][3:]
        sx, sy = c["ships"][0][:2]
        assert (px - sx) ** 2 + (py - sy) ** 2 == d2
    # trajectory cases: the oracle's own predicate on the three geometries
    S = by["traj_left"]["ships"][0][:2]
    assert not pyoracle.enemy_on_trajectory(cfg, S[0], S[1], 700, 1000, 700, 1000)
    assert pyoracle.enemy_on_trajectory(cfg, S[0], S[1], 1300, 1000, 1300, 1000)
    assert pyoracle.enemy_on_trajectory(cfg, S[0], S[1], 1300, 1000, S[0], S[1])
    assert math.atan2(0.0, -300.0) + math.pi == 2 * math.pi
    # order cases: the mover's old place is off the shooter's cone, its new place on it (where it can move at all)
    h, d = sc.ORDER[tag]
    assert d >= ss and 2 + d < W and 1 + h < H
    assert not pyoracle.enemy_on_trajectory(cfg, 2, 1, 2, 2000, 2 + d, 1 + h)
    assert pyoracle.enemy_on_trajectory(cfg, 2, 1, 2, 2000, 2 + d - ss, 1 + h) == (ss > 0)
    assert not pyoracle.enemy_aimed(cfg, 2, 2000, 2 + d - ss, 1 + h)
    assert not pyoracle.enemy_on_trajectory(cfg, 2, 1, 2, 2000, 5000, 1)
    # laser cases: the moving lasers land exactly on the border values
    c = by["laser_borders"]
    below_w = math.nextafter(float(W), 0.0)
    assert c["lasers"][8][0] + sc.device_velocity(1, 0, ls)[0] == float(W)
    gx, gy, gdx, gdy = c["lasers"][9][:4]
    gvx, gvy = sc.device_velocity(gdx, gdy, ls)
    assert (gx + gvx, gy + gvy) == (below_w, 1.5) and below_w < W and (ls == 0 or gvx > 0)
    assert c["lasers"][10][0] + sc.device_velocity(-1, 0, ls)[0] == 0.0
    flight = by["laser_flight"]
    assert flight["expect"][2]["lasers"][0][0] == W // 2 + R + ls
    assert (ls == 0) == (flight["expect"][2]["alive"][0] == 0)          # speed 0: the laser waits on the muzzle
    assert sc.outside(flight["expect"][2]["lasers"][0][0], H // 2, W, H) == (tag in ("tiny", "huge"))


@pytest.mark.parametrize("tag", sc.TAG_NAMES)
def test_raster_scene_on_the_oracle(tag):
    c = sc.raster_scene(tag)
    W, H, r = sc.TAGS[tag]["width"], sc.TAGS[tag]["height"], sc.TAGS[tag]["ship_radius"]
    xs, ys = [s[0] for s in c["ships"]], [s[1] for s in c["ships"]]
    assert min(xs) == min(ys) == 0 and max(xs) == H and max(ys) == W       # [row = y < W][col = x < H]
    assert all(l[0] % 1 == 0.5 and l[1] % 1 == 0.5 for l in c["lasers"])
    sm, lm = sc.plant(tag, c).rasterise()
    assert sm.shape == (W, H) and sm.any() and lm.any()
    assert sm[0, 0] and sm[W - 1, H - 1] and sm[0, H - 1] and sm[W - 1, 0]
    if tag == "huge":
        assert sm.all()                                  # radius 40 on 32 x 32: the discs cover the whole map
    if tag == "tiny":
        assert int(sm.sum()) == 8 and int(lm.sum()) == 15    # radius 1: one cell per ship, four per whole laser
    assert np.array_equal(np.unpackbits(sc.lsb_bits(sm), bitorder="little").reshape(W, H), sm)
