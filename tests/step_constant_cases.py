"""Constant sets, seeded rollouts, crafted boundary cases and raster scenes that hold the lock-step (k_step) and the
rasteriser (k_raster) to the CPU oracle at game constants OTHER than the reference's own 8 / 2 / 8 / 10 and 0 / 0 / 2 / 1.
Not collected: tests/test_step_constant_cases.py checks every scenario's preconditions on the CPU with the oracle alone,
tests/test_gpu_step_constants.py runs the same scenarios on the GPU.

Ships and lasers of the crafted cases are planted (Arena.set_ship / Arena.set_lasers; on the device through
ofx_device_ptr + ofx_memcpy_h2d).  Many of them stand outside the map: only Ship.thrust's clamp and
Battleground.outside look at the map's size, so a case that is about neither is free to use round coordinates.

Every crafted case carries its expectation as numbers written by hand (who lives, each ship's reward as a sum of the
four reward constants, the killing laser's index, a new laser's place and velocity): a mistake shared by the oracle and
the kernel still has to get past them."""
import math

import numpy as np

from oracle import pyoracle

# ---------------------------------------------------------------------------------------------------- constant sets
DEATH, KILL, AIM, TRAJ = -7, 11, 3, 5       # every subset sum is distinct: a ship's reward tells which rules fired
REWARDS = dict(reward_death=DEATH, reward_kill=KILL, reward_aim=AIM, reward_trajectory=TRAJ)
TAGS = {
    "r5": dict(width=64, height=32, ship_radius=3, laser_radius=2, ship_speed=5, laser_speed=5),
    "r13": dict(width=96, height=64, ship_radius=11, laser_radius=2, ship_speed=13, laser_speed=26),
    "r25": dict(width=128, height=64, ship_radius=23, laser_radius=2, ship_speed=0, laser_speed=0),
    "tiny": dict(width=32, height=32, ship_radius=1, laser_radius=1, ship_speed=1, laser_speed=100),
    "huge": dict(width=32, height=32, ship_radius=40, laser_radius=3, ship_speed=3, laser_speed=1),
}
TAG_NAMES = tuple(TAGS)
HIT_RADIUS = {"r5": 5, "r13": 13, "r25": 25, "tiny": 2, "huge": 43}   # R = ship_radius + laser_radius


def constants(tag):
    """The tag's config keywords (ArenaBatch(**kw) and pyoracle.default_cfg(**kw) take the same names)."""
    return dict(TAGS[tag], **REWARDS)


def oracle_cfg(tag, n_ships):
    return pyoracle.default_cfg(n_ships, **constants(tag))


# a reward is KILL * kills + a subset of {DEATH, AIM, TRAJ}; the eight subset sums are distinct modulo KILL
_SUBSETS = {d * DEATH + a * AIM + t * TRAJ: (d, a, t) for d in (0, 1) for a in (0, 1) for t in (0, 1)}


def decode_reward(v):
    """(kills, died, aimed, on_trajectory) of one ship's reward of one lock-step."""
    for kills in range(0, 512):
        if int(v) - KILL * kills in _SUBSETS:
            return (kills,) + _SUBSETS[int(v) - KILL * kills]
    raise ValueError("reward %r is no sum of the reward constants" % (v,))


def hit_threshold(R):
    """The largest double T with sqrt(T) <= R, found with math.sqrt and math.nextafter alone: Circle.collide's
    `distance <= r1 + r2` (form.py:148-149) holds exactly for the squared distances d2 <= T."""
    t = float(R * R)
    while math.sqrt(math.nextafter(t, math.inf)) <= R:
        t = math.nextafter(t, math.inf)
    return t


def threshold_offsets(R):
    """(x_hit, x_miss): a laser at (x, R) from a ship at the origin has the squared distance x*x + R*R, in doubles.
    x_hit makes it exactly T = hit_threshold(R); it is 2**-k where T > R*R (R = 5, 2, 43) and 0 where T is R*R itself
    (R = 13, 25: there one ulp of R*R already carries the root past R).  x_miss makes it the double after T."""
    T, RR = hit_threshold(R), float(R * R)
    x_hit = 0.0
    if T > RR:
        k = 0
        while (2.0 ** -k) * (2.0 ** -k) + RR != T:
            k += 1
            assert k < 80, R
        x_hit = 2.0 ** -k
    after = math.nextafter(T, math.inf)
    j = 0
    while (1.5 * 2.0 ** -j) * (1.5 * 2.0 ** -j) + RR != after:
        j += 1
        assert j < 80, R
    return x_hit, 1.5 * 2.0 ** -j


def device_velocity(dx, dy, speed):
    """Laser.move's velocity for the integer direction (dx, dy) = pointing - fired (laser.py:39-46): what the device
    keeps in F_LASER_DX / F_LASER_DY for a laser that Arena.set_lasers plants by its direction."""
    d = math.sqrt(float(dx * dx + dy * dy))
    return (dx * speed / d, dy * speed / d) if d != 0 else (0.0, 0.0)


def outside(x, y, W, H):
    return (x < 0) or (y < 0) or (x >= W) or (y >= H)      # battleground.py:125-126


def state(o):
    """Everything the oracle knows about one arena, as arrays."""
    s, l = o.ships(), o.lasers()
    return dict(x=s["xy"][:, 0].copy(), y=s["xy"][:, 1].copy(), px=s["pt"][:, 0].copy(), py=s["pt"][:, 1].copy(),
                alive=s["alive"], reward=s["reward"], score=s["score"], killer=s["killer"], hull=s["hull"],
                last_score=s["last_score"], n_lasers=len(l["x"]), lx=l["x"], ly=l["y"], lowner=l["owner"],
                ldead=l["destroyed"])


def lsb_bits(m):
    """A 0/1 map as OFX_MAP_BITS_LSB stores it: cell p is bit p & 31 of the little-endian 32-bit word p >> 5."""
    return np.packbits(np.asarray(m, np.uint8).ravel(), bitorder="little")


# --------------------------------------------------------------------------------------------------- (a) rollouts
ROLLOUT = dict(N=5, M=6, ticks=60, restart_after=25, arena_base=3, spans=(1, 7, 52), map_ticks=(25, 60))
BEHAVIOURS = ("random", "turret", "runner", "shoot", "thrust", "idle")        # one ship per bot law
BOT = dict(idle=0, random=1, turret=2, runner=3, thrust=4, shoot=5)           # OFX_BOT_* (include/ofx.h)
ROLLOUT_SEED = {"r5": 1, "r13": 1, "r25": 15, "tiny": 5, "huge": 71}
EVENTS = ("kill", "laser_hit", "laser_out", "aim", "trajectory")
# what each rollout must contain; the seeds were picked until it does.  laser_hit is a laser destroyed inside the map
# (only a hit does that), laser_out one destroyed outside it in a lock-step in which no hull of its arena changed (only
# Battleground.outside does that).  r25: laser_speed 0, no laser ever leaves the map (one born outside it, off a ship
# at the border, may still be destroyed there: not asked for).  tiny: laser_speed 100 on a 32 x 32 map carries every
# moving laser outside on its first move, so its kills come from the rare laser that never moves (pointing == muzzle).
ROLLOUT_EVENTS = {
    "r5": frozenset(EVENTS),
    "r13": frozenset(EVENTS),
    "r25": frozenset(("kill", "laser_hit", "aim", "trajectory")),
    "tiny": frozenset(EVENTS),
    "huge": frozenset(EVENTS),
}


class OracleRollout:
    """The seeded rollout of a tag on N CPU oracles: bots' actions, lock-step, restart after the 25th lock-step."""

    def __init__(self, tag):
        self.tag, self.N, self.M, self.base = tag, ROLLOUT["N"], ROLLOUT["M"], ROLLOUT["arena_base"]
        self.seed = ROLLOUT_SEED[tag]
        self.W, self.H = TAGS[tag]["width"], TAGS[tag]["height"]
        self.beh = np.array([BOT[x] for x in BEHAVIOURS], np.int32)
        self.oracles = [pyoracle.Arena(cfg=oracle_cfg(tag, self.M)) for _ in range(self.N)]
        for g, o in enumerate(self.oracles):
            o.spawn(pyoracle.reset_draws(o.cfg, self.seed, self.base + g, 0))
        self.t = self.time = self.episode = 0
        self.obs_reward = np.zeros((self.N, self.M), np.int64)     # what F_OBS_REWARD holds: the reward before the step
        self.events = set()

    def restart_due(self):
        return self.t == ROLLOUT["restart_after"] and self.episode == 0

    def restart(self):
        self.episode += 1
        self.time = 0
        for g, o in enumerate(self.oracles):
            o.restart(pyoracle.reset_draws(o.cfg, self.seed, self.base + g, self.episode))

    def actions(self):
        return [o.bot_actions(self.beh, self.seed, self.base + g, self.t) for g, o in enumerate(self.oracles)]

    def step(self, acts):
        for g, o in enumerate(self.oracles):
            before = o.ships()
            self.obs_reward[g] = before["reward"]
            o.step(acts[g])
            after, l = o.ships(), o.lasers()
            if ((before["alive"] == 1) & (after["alive"] == 0)).any():
                self.events.add("kill")
            nobody_hit = np.array_equal(before["hull"], after["hull"])
            for x, y, dead in zip(l["x"], l["y"], l["destroyed"]):
                if dead and not outside(x, y, self.W, self.H):
                    self.events.add("laser_hit")
                elif dead and nobody_hit:
                    self.events.add("laser_out")
            for v in after["reward"]:
                _, _, aimed, traj = decode_reward(v)
                if aimed:
                    self.events.add("aim")
                if traj:
                    self.events.add("trajectory")
        self.t += 1
        self.time += 1


# ------------------------------------------------------------------------------------------------ (b) crafted cases
NOOP = (0, 0, 0, 0, 0)                       # valid = 0: the reference's None
FAR, FAR2 = (5000, 5000), (6000, 5000)       # bystanders: in nobody's reach, cone or aim
# integer (a, b) with a*a + b*b == R*R, 0 <= a <= b: R = 5, 13, 25 are hypotenuses; 2 and 43 only have (0, R)
TRIPLE = {5: (3, 4), 13: (5, 12), 25: (7, 24), 2: (0, 2), 43: (0, 43)}
AIM_TRIPLE = {40: (24, 32)}                  # of the ship radii 3, 11, 23, 1, 40 only 40 is a hypotenuse
# "order" cases, inside the map because Ship.thrust clamps: the shooter at (2, 1) fires straight up; the mover stands h
# up and d to the right of that line and thrusts ship_speed toward it.  (h, d): d is off the shooter's cone (half-width
# atan(ship_radius / distance)) and d - ship_speed is on it; r25 cannot move.
ORDER = {"r5": (30, 5), "r13": (60, 13), "r25": (60, 30), "tiny": (30, 1), "huge": (2, 10)}
# thrust from (10, 10) toward (13, 14) and toward (7, 6): 10 +- int-truncated 0.6 and 0.8 of the speed 5, 13, 0, 1, 3
THRUST_345 = {"r5": (13, 14), "r13": (17, 20), "r25": (10, 10), "tiny": (10, 10), "huge": (11, 12)}
THRUST_NEG = {"r5": (7, 6), "r13": (2, 0), "r25": (10, 10), "tiny": (9, 9), "huge": (8, 7)}
# a shot along +x from the map's centre, one lock-step after the shot: the laser's x = W/2 + R + laser_speed, whether
# it is destroyed (outside, or - r25, speed 0 - still on the muzzle at distance exactly R of its owner), and the
# shooter's alive flag and reward
LASER_FLIGHT = {"r5": (42.0, 0, 1, 0), "r13": (87.0, 0, 1, 0), "r25": (89.0, 1, 0, KILL + DEATH),
                "tiny": (118.0, 1, 1, 0), "huge": (60.0, 1, 1, 0)}


def _ship(xy, pt=None):
    return (xy[0], xy[1]) + (tuple(pt) if pt is not None else (xy[0], xy[1]))


def _still(x, y, owner):
    return (float(x), float(y), 0, 0, owner, 0)        # a laser that never moves


def crafted_cases(tag):
    """The tag's cases: dicts of name, ships [(x, y, px, py)], lasers [(x, y, dx, dy, owner, destroyed)] with the
    integer direction of Arena.set_lasers, actions (two lock-steps of one (valid, shoot, thrust, px, py) per ship) and
    expect {lock-step: {field: values}} with the fields of state() plus `xy`, `lasers` [(x, y)] and `vel` [(dx, dy)],
    the device's F_LASER_DX / F_LASER_DY."""
    c = TAGS[tag]
    W, H, r, ss, ls = c["width"], c["height"], c["ship_radius"], c["ship_speed"], c["laser_speed"]
    R = HIT_RADIUS[tag]
    a, b = TRIPLE[R]
    x_hit, x_miss = threshold_offsets(R)
    out = []

    def case(name, ships, lasers=(), first=None, expect=None):
        M = len(ships)
        acts = [list(first) if first is not None else [NOOP] * M, [NOOP] * M]
        assert len(acts[0]) == M
        out.append(dict(name=name, M=M, ships=[tuple(s) for s in ships], lasers=[tuple(l) for l in lasers],
                        actions=acts, expect=expect or {}))

    # ---- hit threshold: the missing laser comes FIRST in the list, so a wrong hit shows in the killer's index too
    case("hit_integer", [_ship((0, 0)), _ship(FAR)], [_still(a, b + 1, 1), _still(b, a, 1)],
         expect={1: dict(alive=[0, 1], reward=[DEATH, KILL], killer=[1, -1])})
    case("hit_threshold", [_ship((0, 0)), _ship(FAR)], [_still(x_miss, R, 1), _still(x_hit, R, 1)],
         expect={1: dict(alive=[0, 1], reward=[DEATH, KILL], killer=[1, -1])})
    case("multikill", [_ship((0, 0)), _ship((2 * a, 2 * b)), _ship(FAR)], [_still(a, b, 2)],
         expect={1: dict(alive=[0, 0, 1], reward=[DEATH, DEATH, 2 * KILL], killer=[0, 0, -1], ldead=[1])})
    case("two_lasers", [_ship((0, 0)), _ship(FAR), _ship(FAR2)], [_still(a, b, 2), _still(b, a, 1)],
         expect={1: dict(alive=[0, 1, 1], reward=[DEATH, 0, KILL], killer=[0, -1, -1])})
    # ---- aim: the enemy at distance exactly ship_radius of the pointing, and one past it.  The shooter fires straight
    # up at an enemy on its own column, so the trajectory reward comes with every one of these shots
    foe = (1000, 500)
    for name, off, rew in (("aim_at_r", (0, r), AIM + TRAJ), ("aim_past_r", (0, r + 1), TRAJ)):
        case(name, [_ship((1000, 0)), _ship(foe)], first=[(1, 1, 0, foe[0] + off[0], foe[1] + off[1]), NOOP],
             expect={1: dict(alive=[1, 1], reward=[rew, 0], n_lasers=1)})
    if r in AIM_TRIPLE:
        ta, tb = AIM_TRIPLE[r]
        for name, off, rew in (("aim_triple", (ta, tb), AIM + TRAJ), ("aim_past_triple", (ta, tb + 1), TRAJ)):
            case(name, [_ship((1000, 0)), _ship(foe)], first=[(1, 1, 0, foe[0] + off[0], foe[1] + off[1]), NOOP],
                 expect={1: dict(alive=[1, 1], reward=[rew, 0], n_lasers=1)})
    # ---- pointing on the rim of the own hit-box (d2 == inR^2: fired = the ship's centre, the laser starts ON the
    # pointing and still flies) and one past it at (1, R) (fired = the muzzle (0, R - 1): it flies along (1, 1))
    S = (1000, 1000)
    case("hitbox_on", [_ship(S), _ship(FAR)], first=[(1, 1, 0, S[0] + a, S[1] + b), NOOP],
         expect={1: dict(reward=[0, 0], lasers=[(S[0] + a, S[1] + b)], vel=[(a * ls / R, b * ls / R)])})
    case("hitbox_past", [_ship(S), _ship(FAR)], first=[(1, 1, 0, S[0] + 1, S[1] + R), NOOP],
         expect={1: dict(reward=[0, 0], lasers=[(S[0], S[1] + R - 1)], vel=[(ls / math.sqrt(2.0), ls / math.sqrt(2.0))])})
    # ---- trajectory: due left the target angle is 2 pi and the cone wraps: never a hit (ship.py:203-208); due right
    # it is pi; on the shooter's own cell the distance is 0, the angular radius 2 pi and both bounds come out as pi
    case("traj_left", [_ship(S), _ship((700, 1000))], first=[(1, 1, 0, 700, 1000), NOOP],
         expect={1: dict(alive=[1, 1], reward=[AIM, 0])})
    case("traj_right", [_ship(S), _ship((1300, 1000))], first=[(1, 1, 0, 1300, 1000), NOOP],
         expect={1: dict(alive=[1, 1], reward=[AIM + TRAJ, 0])})
    case("traj_same_cell", [_ship(S), _ship(S)], first=[(1, 1, 0, 1300, 1000), NOOP],
         expect={1: dict(alive=[1, 1], reward=[TRAJ, 0])})
    # ---- ships move in index order: shooter 1 sees the NEW place of mover 0 and the OLD place of mover 2
    h, d = ORDER[tag]
    gun, aim_up = (2, 1), (2, 2000)
    mover, moved = _ship((2 + d, 1 + h), (2, 1 + h)), (2 + d - ss, 1 + h)
    bystander = _ship((5000, 1))
    case("order_lower_index", [mover, _ship(gun), bystander],
         first=[(1, 0, 1, 2, 1 + h), (1, 1, 0) + aim_up, NOOP],
         expect={1: dict(reward=[0, TRAJ if ss > 0 else 0, 0], xy=[moved, gun, (5000, 1)])})
    case("order_higher_index", [bystander, _ship(gun), mover],
         first=[NOOP, (1, 1, 0) + aim_up, (1, 0, 1, 2, 1 + h)],
         expect={1: dict(reward=[0, 0, 0], xy=[(5000, 1), gun, moved])})
    # ---- thrust
    case("thrust_overshoot", [_ship((5, 5)), _ship(FAR)], first=[(1, 0, 1, 6, 5), NOOP],       # the pointing is 1 away
         expect={1: dict(xy=[(5 + ss, 5), FAR], px=[6, FAR[0]], py=[5, FAR[1]])})
    case("thrust_345", [_ship((10, 10)), _ship(FAR)], first=[(1, 0, 1, 13, 14), NOOP],
         expect={1: dict(xy=[THRUST_345[tag], FAR])})
    case("thrust_neg", [_ship((10, 10)), _ship(FAR)], first=[(1, 0, 1, 7, 6), NOOP],
         expect={1: dict(xy=[THRUST_NEG[tag], FAR])})
    case("thrust_low_border", [_ship((2, 7)), _ship((7, 2))], first=[(1, 0, 1, -100, 7), (1, 0, 1, 7, -100)],
         expect={1: dict(xy=[(max(0, 2 - ss), 7), (7, max(0, 2 - ss))])})
    case("thrust_high_border", [_ship((W - 2, 5)), _ship((5, H - 2))],
         first=[(1, 0, 1, W + 100, 5), (1, 0, 1, 5, H + 100)],
         expect={1: dict(xy=[(min(W - 1, W - 2 + ss), 5), (5, min(H - 1, H - 2 + ss))])})
    case("thrust_nowhere", [_ship((10, 10)), _ship(FAR)], first=[(1, 1, 1, 10, 10), NOOP],     # pointing == position
         expect={1: dict(xy=[(10, 10), FAR], reward=[0, 0], n_lasers=0)})
    # ---- lasers
    fx, fdead, falive, frew = LASER_FLIGHT[tag]
    cx, cy = W // 2, H // 2
    case("laser_flight", [_ship((cx, cy)), _ship(FAR)], first=[(1, 1, 0, cx + 1000, cy), NOOP],
         expect={1: dict(lasers=[(cx + R, cy)], vel=[(float(ls), 0.0)], ldead=[0], reward=[0, 0]),
                 2: dict(lasers=[(fx, cy)], ldead=[fdead], alive=[falive, 1], reward=[frew, 0])})
    below_w, below_h, below_0 = math.nextafter(float(W), 0.0), math.nextafter(float(H), 0.0), -5e-324
    # the laser that lands on the last double below W: along +x, but for tiny along (7, 24) - 28 a lock-step in x,
    # 96 in y - because a start 100 to the left of the map is too coarse a double to land there
    gdx, gdy = (7, 24) if tag == "tiny" else (1, 0)
    gvx, gvy = device_velocity(gdx, gdy, ls)
    case("laser_borders", [_ship(FAR), _ship(FAR2)],
         [_still(W, 1.5, 0), _still(below_w, 1.5, 0), _still(1.5, H, 0), _still(1.5, below_h, 0),
          _still(0.0, 1.5, 0), _still(below_0, 1.5, 0), _still(1.5, 0.0, 0), _still(1.5, below_0, 0),
          (float(W - ls), 1.5, 1, 0, 0, 0), (below_w - gvx, 1.5 - gvy, gdx, gdy, 0, 0), (float(ls), 1.5, -1, 0, 0, 0)],
         expect={1: dict(alive=[1, 1], reward=[0, 0], ldead=[1, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0],
                         lasers=[(W, 1.5), (below_w, 1.5), (1.5, H), (1.5, below_h), (0.0, 1.5), (below_0, 1.5),
                                 (1.5, 0.0), (1.5, below_0), (W, 1.5), (below_w, 1.5), (0.0, 1.5)])})
    return out


def raster_scene(tag):
    """(c) one arena that is only drawn: ships on the four borders, in the corners and one past the far corner, and
    still lasers centred at k + 0.5, inside, across the borders and outside.  The map is [row = y < W][col = x < H]
    (observation.py:86, form.py:226), so the borders are those of that array."""
    W, H = TAGS[tag]["width"], TAGS[tag]["height"]
    ships = [(0, 0), (H - 1, 0), (0, W - 1), (H - 1, W - 1), (H // 2, 0), (H // 2, W - 1), (0, W // 2),
             (H - 1, W // 2), (H, W)]
    lasers = [(0.5, 0.5), (H - 0.5, W - 0.5), (H // 2 + 0.5, 0.5), (-0.5, W // 2 + 0.5), (H + 0.5, 3.5), (7.5, 9.5)]
    return dict(name="raster_scene", M=len(ships), ships=[_ship(s) for s in ships],
                lasers=[_still(x, y, 0) for x, y in lasers], actions=[], expect={})


def plant(tag, case):
    """The case's start on a fresh oracle."""
    o = pyoracle.Arena(cfg=oracle_cfg(tag, case["M"]))
    o.spawn(np.zeros((case["M"], 2), np.int32))
    for i, s in enumerate(case["ships"]):
        o.set_ship(i, *s)
    L = case["lasers"]
    o.set_lasers(*[[l[k] for l in L] for k in range(6)])
    return o


def check_expectation(case, step, st, vel=None):
    """Hold state `st` (state() of the oracle, or the same fields read from the device) after lock-step `step` to the
    case's hand-written numbers.  vel = the lasers' (dx, dy) where the caller has them (the device)."""
    for key, want in case["expect"].get(step, {}).items():
        where = (case["name"], step, key)
        if key == "xy":
            assert [(int(x), int(y)) for x, y in zip(st["x"], st["y"])] == [tuple(w) for w in want], where
        elif key == "lasers":
            got = [(float(x), float(y)) for x, y in zip(st["lx"], st["ly"])]
            assert len(got) == len(want), where
            for g, w in zip(got, want):            # == on floats, and the sign of a zero
                assert g == (float(w[0]), float(w[1])) and math.copysign(1, g[0]) == math.copysign(1, w[0]), where + (g, w)
        elif key == "vel":
            if vel is not None:
                assert [(float(x), float(y)) for x, y in vel] == [(float(x), float(y)) for x, y in want], where + (vel,)
        elif key == "n_lasers":
            assert int(st["n_lasers"]) == want, where
        else:
            assert [int(v) for v in st[key]] == list(want), where + (list(st[key]),)
