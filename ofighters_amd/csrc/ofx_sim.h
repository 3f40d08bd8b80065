// ofx_sim.h - the arena rules that more than one kernel applies, each stated once (device-inline; included at the end
// of ofx_internal.h).  They convert integers and evaluate the counter RNG: no floating-point product feeds a sum
// here, so the translation unit's -ffp-contract setting cannot reach them.
#pragma once

// The scripted bots' law for ship `i` of global arena `ga` at lock-step `tick` (agents/agent.py:99-155 on the counter
// RNG).  `alive` / (ptx, pty) are the ship's state when request_actions runs, i.e. before that lock-step's lasers move
// (battleground.py:146-150); a dead ship's agent is still stepped but its action is None (ship.py:260-262).
__device__ inline ofx_action ofx_bot_action(int beh, uint32_t ga, uint32_t i, uint32_t tick, ofx_rng_key key, int W, int H,
                                            bool alive, int ptx, int pty) {
  uint32_t r[4];
  ofx_philox4x32_10(ga, i, tick, OFX_STREAM_BOT, key, r);
  bool shoot = false, thrust = false, repoint = false;
  const double u0 = ofx_unit(r[0]), u1 = ofx_unit(r[1]);
  switch (beh) {
    case OFX_BOT_RANDOM: {
      const uint32_t k = (uint32_t)(((uint64_t)r[0] * 3u) >> 32);
      shoot = k == 0; thrust = k == 1; repoint = k == 2;
    } break;
    case OFX_BOT_TURRET: shoot = u0 < 0.8; repoint = u1 < 0.3; break;
    case OFX_BOT_RUNNER: thrust = u0 < 0.9; repoint = u1 < 0.1; break;
    case OFX_BOT_THRUST: thrust = true; break;
    case OFX_BOT_SHOOT: shoot = true; break;
    default: break;
  }
  ofx_action act;
  act.px = ptx; act.py = pty;
  act.shoot = 0; act.thrust = 0; act.valid = alive ? 1 : 0; act._pad = 0;
  if (alive) {
    act.shoot = shoot; act.thrust = thrust;
    if (repoint) { act.px = ofx_draw_int(r[2], W); act.py = ofx_draw_int(r[3], H); }
  }
  return act;
}

// The restart draws (dx, dy) of ship `i` of global arena `ga` in episode `episode` (episode 0: the spawn)
__device__ inline void ofx_reset_draw(ofx_rng_key key, int W, int H, uint32_t ga, uint32_t i, uint32_t episode, int *dx,
                                      int *dy) {
  uint32_t r[4];
  ofx_philox4x32_10(ga, i, episode, OFX_STREAM_RESET, key, r);
  *dx = ofx_draw_int(r[0], W);
  *dy = ofx_draw_int(r[1], H);
}

// The eight scalars that lead Observation.toVector for ship s = a * M + i on a W x H map (observation.py:101-123).
// The reward is st.reward, not st.obs_reward: the observation is made after generate_frame and before the next
// Agent.step adds the reward to the score and zeroes it.
template <class T>
__device__ inline void ofx_obs_head(const ofx_state &st, int s, int W, int H, T v[8]) {
  v[0] = (T)st.reward[s];
  v[1] = 1;  // can_shoot is constant 1 (ship.py:58)
  v[2] = (T)st.ship_px[s];
  v[3] = (T)st.ship_py[s];
  v[4] = (T)W;
  v[5] = (T)H;
  v[6] = (T)st.ship_x[s];
  v[7] = (T)st.ship_y[s];
}
