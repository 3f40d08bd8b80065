"""Sharded rollout driver: the host logic of the N>1 path.

Arenas never interact (all state is per Battleground; the only cross-arena
object of the reference is the read-only policy singleton,
agents/qlearnIA_V2.py:308,342), so the path shards trivially: rank r of W owns
the contiguous block of global arenas [r*n, (r+1)*n).  The counter RNG is keyed
by the GLOBAL arena id, so any world size reproduces the same arenas.  The one
collective is the all-reduce of the per-slot episode scores banked by
Agent.reset (agents/agent.py:61-63) at each episode end - RCCL over xGMI on the
GPUs (backend "nccl"), gloo in the CPU tests.

The engine is duck-typed (ArenaBatch on the GPU; tests drive the same code with
an oracle-backed stand-in under gloo, world_size 2).
"""
import numpy as np


def shard_range(rank, world, arenas_per_rank):
    """(first global arena id, count) of a rank's shard - weak scaling."""
    if not (0 <= rank < world):
        raise Exception("rank %d outside world of %d" % (rank, world))
    return rank * arenas_per_rank, arenas_per_rank


class ShardedRollout:
    """Lock-step loop of one shard: actions -> step -> observation, episode
    restarts every `episode_ticks` (lib/ofighters.py:59,684-688) and the
    episodic score all-reduce.

    engine   object with spawn_random / restart_random / bot_actions / step /
             rasterise / episode_scores(as int64 numpy [M+1]) and attributes
             N, M, episode (ArenaBatch on the GPU - bench.py drives THIS class at every
             world size - or the oracle-backed stand-in of the gloo test)
    dist     a torch.distributed-like module or None (single process)
    """

    def __init__(self, engine, behaviours, seed, episode_ticks=200, dist=None, observe=True, policy=None,
                 to_tensor=None, start_tick=0, probe=None, use_rollout=False):
        self.e = engine
        self.behaviours = list(behaviours)
        self.seed = seed
        self.episode_ticks = episode_ticks
        self.dist = dist
        self.observe = observe
        self.policy = policy          # callable(engine) -> None: overwrite the policy ships' actions
        self.to_tensor = to_tensor    # numpy [M+1] int64 -> tensor usable by dist.all_reduce
        self.probe = probe            # callable(stage, begin[, n_ticks]) around "step" / "obs" (bench.py) or None
        self.use_rollout = use_rollout  # without a policy: K lock-steps per host call through engine.rollout
        self.tick = start_tick        # a start inside an episode puts its end where the caller wants it (bench.py)
        self.score_log = []           # all-reduced [M+1] per finished episode
        self.e.spawn_random(seed)

    def _episode_end(self):
        self.e.restart_random(self.seed)
        local = np.asarray(self.e.episode_scores(), dtype=np.int64)
        if self.dist is not None:
            t = self.to_tensor(local)
            self.dist.all_reduce(t)           # SUM over ranks: the only collective of the path
            total = np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t, dtype=np.int64)
        else:
            total = local
        self.score_log.append(total.copy())
        return total

    def lockstep(self):
        if self.tick > 0 and self.tick % self.episode_ticks == 0:
            self._episode_end()
        self._fly_and_step()

    def _fly_and_step(self):
        """A lock-step behind its episode-end check: the bots, the policy hook, the step, the observation."""
        self.e.bot_actions(self.behaviours, self.seed, tick=self.tick)
        if self.policy is not None:
            self.policy(self.e)
        p = self.probe
        if p: p("step", True)
        self.e.step()
        if p: p("step", False)
        if self.observe:
            if p: p("obs", True)
            self.e.rasterise()
            if p: p("obs", False)
        self.tick += 1

    def run(self, ticks):
        if self.policy is None and self.use_rollout and hasattr(self.e, "rollout"):
            return self._run_headless(ticks)
        for _ in range(ticks):
            self.lockstep()
        return self.score_log

    def _run_headless(self, ticks):
        """Scripted bots only: whole runs of lock-steps up to the next episode end go down in ONE host call
        (ofx_rollout, the batched Battleground.run of battleground.py:169-173); the restart + score all-reduce at the
        episode ends are the same code as in lockstep()."""
        from . import _native as nat
        left = ticks
        while left > 0:
            if self.tick > 0 and self.tick % self.episode_ticks == 0:
                self._episode_end()
            n = min(left, self.episode_ticks - self.tick % self.episode_ticks)
            p = self.probe
            stage = "obs" if self.observe else "step"
            if p: p(stage, True, n)     # n lock-steps go down in this one call
            self.e.rollout(self.behaviours, self.seed, self.tick, n, nat.MAP_U8 if self.observe else None)
            if p: p(stage, False, n)
            self.tick += n
            left -= n
        return self.score_log


class TrainingRollout(ShardedRollout):
    """The learning agent as a whole: `QlearnIA.play` + `Trainer` (agents/qlearnIA_V2.py:372-418, 199-287) for every
    policy ship of every arena of the shard, in lock-step, all on the device.

    One lock-step =
        scripted bots for the other ships                                      agent.py:99-155
        forward on the trainer's (pinned) weights -> epsilon-greedy / the      :397, :199-235
          collecting phase's random play (first `collecting_steps` steps)      :393-395
          (trainer.actor_priorities: one call that also returns the values of the choice; the capture below
          turns them into the new rows' priorities - same actions, same rows)
        transition capture (remember previous_obs ... obs, done latch)         :388-391, :401-403
        action packing, step, rasterise                                        :447-454, battleground.py:153-166
        epsilon decay (once per lock-step: "all bots share the same trainer")  :398-400
        `trainer.replay(batch_size)` every `replay_every` total steps          :414-415  (total_steps % 50 == 0)
          and on the lock-steps where a learning agent first sees its death    :376-378
        a snapshot every `snapshot_every` episodes                             :416-417
        a checkpoint every `checkpoint_every` episodes (not in the reference; off by default)

    A snapshot is the trainer's weights alone (DeviceTrainer.save, the Keras-compatible .npz).  `checkpoint(path)` writes
    everything the run needs to go on in another process - arenas, replay memory, optimiser, counters
    (ofighters_amd/checkpoint.py) - and `restore(path)`, called on a freshly constructed TrainingRollout built with the
    same arguments on a fresh ArenaBatch + DeviceTrainer, continues it bit for bit.  With `checkpoint_every=K` and a
    `checkpoint_folder`, the lock-step that completes every K-th episode ends by writing `<folder>/checkpoint-latest`,
    replacing the previous one (the episode's restart is then the first thing the restored run does).

    The reference calls replay once per dying agent; the batched form does at most ONE replay per lock-step (its
    minibatch already draws from every arena's memory), on `DeviceTrainer.fit_batch` rows of what it sampled.  After a fit the trainer's blob has changed in place and
    libofx re-prepares the pinned copy itself (ofx_dqn_fit -> ofx_policy_weights_updated), so the next forward plays
    with the new weights like Keras' shared model does.

    Opt-in, not in the reference (ofighters_amd/exploration.py; Horgan et al. 2018, Ape-X): `epsilon_ladder=alpha` gives
    every arena its own exploration rate, global arena g of the L learning arenas playing at
    epsilon ** (1 + alpha * g / (L - 1)), and `eval_arenas=k` makes the last k global arenas of the run greedy: the forward
    still plays them (under the full policy mask) on the current weights, but they never explore, and a second device
    mask - the policy mask with those arenas zeroed - keeps them out of the capture (their memories stay empty: greedy
    play is not the behaviour policy the learner samples) and out of the death count that triggers a replay.
    `total_arenas` is the run's number of arenas over all shards (default: engine.N; a sharded run passes the world's
    total, the ladder is keyed by engine.arena_base + a).  With either option on, every episode end also appends the
    int64 [G][M+1] of engine.episode_scores_grouped to `rung_log` (all-reduced like score_log): the learning arenas in
    `score_bands` contiguous bands by global id - clipped to the learning arenas and to the n_groups <= N one shard can
    count - then, with eval_arenas, the evaluation group; `eval_scores` lists per episode the mean banked score of a
    policy ship of an evaluation arena - the one number that shows whether the current weights play better.  eval_arenas
    alone leaves every learning arena at exponent 1.  With both off, _play makes exactly the calls it always made.

    Opt-in, not in the reference (Mnih et al. 2015, "frame skip"): `action_repeat=K` (an integer >= 1, 1 = off) makes one
    `lockstep()` one DECISION that is held for K lock-steps.  The episode-end check and `_play` run as they are, then ONE
    engine.step_repeat (ofx_step_repeat: K lock-steps inside one kernel launch, the policy ships on the action just
    packed, the others on the bots' law lock-step by lock-step, the maps rasterised once at the end) stands where
    bot_actions + step + rasterise stood, and `tick` advances by K.  The rollout owns an int32 [N][M] device buffer that
    receives every ship's rewards summed over the span (undiscounted) and registers it with engine.replay_reward_source:
    the row the next capture completes carries the whole span's reward, while element 0 of the stored observation head
    stays the state's reward, as the live forward sees it.  Under action_repeat `total_steps`, `collecting_steps`,
    `replay_every`, the epsilon schedule, `capture_tick` and the argument of run() all count DECISIONS, not lock-steps;
    `episode_ticks`, `tick` and the bots' counter ticks stay lock-steps.  K must divide `episode_ticks` and `start_tick`
    (a span never crosses an episode end): ValueError before the first device call otherwise.  With K == 1 none of this
    exists and lockstep() / _play make exactly the calls they always made.

    Opt-in, not in the reference (every vectorised RL environment restarts a sub-environment when ITS episode ends):
    `auto_reset=True` (a bool; anything else is a ValueError before the first device call) gives every arena its own
    episodes.  Without it all arenas restart together every `episode_ticks` lock-steps, and an arena whose learning ship
    was destroyed early pays the forward for the rest of the episode without capturing a row.  With it every lockstep()
    - every decision under action_repeat - STARTS with engine.restart_finished (ofx_restart_finished: one kernel, nothing
    comes back to the host) on the full policy mask, so evaluation arenas restart on their ships' deaths too: an arena
    restarts when all its policy ships are finished or its own clock has reached `episode_ticks`, on the draws of its own
    episode counter; its `_seen_done` latches and its agents' previous_* / done latch are cleared on the device
    (`_seen_done` is never zeroed from the host, restart_random is never called after the spawn).  A destroyed ship is
    finished on the SECOND call that sees it dead: the lock-step in between is the one in which _play counts the death,
    replays and captures the losing frame (done = 1), the reference's order (agents/qlearnIA_V2.py:376-391) - so an arena
    restarts one lock-step after its last learner's death was seen, not on that lock-step.  What the restarts bank - per
    group under the ladder / evaluation options, else in one row - accumulates on the device in a rollout-owned int64
    [G][M+2]: M scores, the episodes, their lock-steps.  `tick % episode_ticks == 0` (tick > 0) is then the end of a
    REPORTING PERIOD, nothing restarts because of it: the sums are downloaded, zeroed and all-reduced like score_log, and
    appended - columns 0..M summed over the groups to `score_log` (index M: the episodes that ended in the period, no
    longer the arena count), the [G][M+1] block to `rung_log` under the ladder options, column M+1 as [G] to `length_log`
    (lock-steps of the finished episodes; over the episodes = the mean episode length).  `episode`, `epsilons`,
    `snapshot_every` and `checkpoint_every` count reporting periods; `eval_scores` keeps its formula (index M is still
    the episode count).  engine.episode stays 0: the arenas' counters are engine.autoreset_state()["arena_episode"].
    Under action_repeat = K an arena's clock advances by K per decision and K divides episode_ticks, so the clock still
    ends an episode exactly there.  The trainer does not change: n-step chains stop at the cleared previous_*.  With
    auto_reset=False none of this exists and lockstep() makes exactly the calls it always made.

    Opt-in, not in the reference (Boltzmann / softmax exploration, e.g. Sutton & Barto 2018, section 2.8):
    `boltzmann=(tau_act, tau_ptr)`, a pair of finite floats >= 0 (anything else: ValueError naming `boltzmann` before the
    first device call).  An exploring ship of the default rule points uniformly over all 160 000 cells; with the option
    every policy ship SAMPLES both heads from softmax(Q / T), T = tau * eps_a with eps_a the arena's exploration rate:
    the trainer's epsilon schedule anneals the temperature, the ladder spreads it over the arenas and the evaluation
    arenas (exponent +inf, T = 0) stay greedy.  _play then makes ONE engine.policy_act_boltzmann call
    (ofx_policy_act_boltzmann: the pointer is sampled inside the streaming head kernel by the Gumbel-max identity, on
    noise keyed by pixel and `capture_tick`) where forward + explore - or policy_act under actor_priorities - stood,
    followed by the same capture.  The collecting phase is the default rule's, bit for bit.  No new state: a checkpoint
    carries the pair in its fingerprint only.  With boltzmann=None _play makes exactly the calls it always made.

    engine    ArenaBatch
    trainer   DeviceTrainer built on that engine (owns weights, Adam state, epsilon, the replay memory)
    policy_ships  ship slots driven by the policy (the stock line-up has ONE, lib/ofighters.py:53); the others
              follow `behaviours`
    """

    def __init__(self, engine, trainer, behaviours, seed, policy_ships=(0,), is_learning=True, collecting_steps=20,
                 replay_every=50, replay_on_death=True, snapshot_every=50, snapshot_folder=None, checkpoint_every=0,
                 checkpoint_folder=None, epsilon_ladder=None, eval_arenas=0, total_arenas=None, score_bands=8,
                 action_repeat=1, auto_reset=False, boltzmann=None, **kw):
        from . import exploration
        self.boltzmann = exploration.boltzmann_pair(boltzmann)   # every argument is checked before the first device call
        if not isinstance(auto_reset, (bool, np.bool_)):   # every argument is checked before the first device call
            raise ValueError("auto_reset must be a bool, got %r" % (auto_reset,))
        self.auto_reset = bool(auto_reset)
        self.action_repeat = exploration._integer("action_repeat", action_repeat, 1)
        if self.action_repeat > 1:                 # every argument is checked before the first device call
            for name, default in (("episode_ticks", 200), ("start_tick", 0)):
                v = exploration._integer(name, kw.get(name, default), 0)
                if v % self.action_repeat:
                    raise ValueError("action_repeat = %d must divide %s = %d (a span never crosses an episode end)"
                                     % (self.action_repeat, name, v))
        self.ladder_on = epsilon_ladder is not None or isinstance(eval_arenas, bool) or eval_arenas != 0
        self.epsilon_ladder, self.eval_arenas = None, 0
        if self.ladder_on:                         # every argument is checked before the first device call
            total = engine.N if total_arenas is None else total_arenas
            expo = exploration.apex_exponents(total, 0.0 if epsilon_ladder is None else epsilon_ladder, engine.arena_base,
                                              engine.N, eval_arenas)
            learning = int(total) - int(eval_arenas)
            exploration._integer("score_bands", score_bands, 1)
            bands = min(int(score_bands), learning, engine.N - (1 if eval_arenas else 0))
            if bands < 1:
                raise ValueError("eval_arenas needs at least 2 arenas per shard for the grouped scores, got %d" % engine.N)
            groups = exploration.score_groups(total, engine.arena_base, engine.N, bands, eval_arenas)
            self.epsilon_ladder = None if epsilon_ladder is None else float(epsilon_ladder)
            self.eval_arenas, self.total_arenas, self.score_bands = int(eval_arenas), int(total), bands
            self.n_groups = exploration.n_groups(bands, eval_arenas)
        super().__init__(engine, behaviours, seed, **kw)
        self.trainer = trainer
        self.is_learning = bool(is_learning)
        self.collecting_steps = collecting_steps
        self.replay_every = replay_every
        self.replay_on_death = bool(replay_on_death)
        self.snapshot_every = snapshot_every
        self.snapshot_folder = snapshot_folder     # None: no files are written
        self.checkpoint_every = checkpoint_every   # 0: no checkpoints
        self.checkpoint_folder = checkpoint_folder
        self.total_steps = 0                       # Agent.total_steps of the learning agents (agent.py:68)
        self.episode = 0
        self.losses = []                           # QlearnIA.losses: history['loss'][0] = mse(output1) + mse(output2)
        self.epsilons = []                         # QlearnIA.epsilons: one per episode (:364-365)
        self.snapshots = []
        from .engine import DeviceBuffer
        mk = np.zeros((engine.N, engine.M), np.uint8)
        mk[:, list(policy_ships)] = 1
        self.policy_mask = mk
        engine.sync()
        self._mask = DeviceBuffer(mk.nbytes).upload(mk)
        self._learn_mask = self._mask              # what captures and counts deaths: the policy ships of learning arenas
        self.rung_log = []                         # all-reduced [G][M+1] per finished episode (ladder / eval arenas only)
        if self.ladder_on:
            if self.eval_arenas:
                lm = mk.copy()
                lm[np.isinf(expo)] = 0
                self._learn_mask = DeviceBuffer(lm.nbytes).upload(lm)
            self._groups = DeviceBuffer(groups.nbytes).upload(groups)
            engine.policy_epsilon_ladder(expo)
        self._zeros = np.zeros((engine.N, engine.M), np.uint8)
        self._seen_done = DeviceBuffer(mk.nbytes).upload(self._zeros)   # the agents' `done` latches, on the device
        engine.policy_pin_weights(trainer.weights.ptr)
        self.policy = self._play
        self.capture_tick = 0                      # ofx_replay_capture's clock: never restarts at episode ends
        if self.action_repeat > 1:
            # every ship's rewards summed over the last span: what the next capture's completed rows carry
            span = np.zeros((engine.N, engine.M), np.int32)
            self._span = DeviceBuffer(span.nbytes).upload(span)
            engine.replay_reward_source(self._span.ptr)
        self.length_log = []                       # all-reduced [G] per reporting period: lock-steps of finished episodes
        if self.auto_reset:
            # what the restarts of a reporting period bank, per group: M scores, the episodes, their lock-steps
            self._auto_groups = self.n_groups if self.ladder_on else 1
            self._auto_zero = np.zeros((self._auto_groups, engine.M + 2), np.int64)
            self._auto_sums = DeviceBuffer(self._auto_zero.nbytes).upload(self._auto_zero)
            # the engine's counters exist from here on: a checkpoint may be written before the first lock-step
            engine.load_autoreset_state({"arena_episode": np.zeros(engine.N, np.uint32),
                                         "dead_once": np.zeros((engine.N, engine.M), np.uint8)})

    def _restart_finished(self):
        """The head of a lock-step under auto_reset: the arenas whose policy ships are all finished, or whose clock
        has reached episode_ticks, restart on the device."""
        self.e.restart_finished(self.seed, self._mask.ptr, max_ticks=self.episode_ticks, seen_buf=self._seen_done,
                                group_buf=self._groups if self.ladder_on else None, n_groups=self._auto_groups,
                                sums_buf=self._auto_sums)

    def _period_end(self):
        """auto_reset: `tick` reached a multiple of episode_ticks - report what the restarts since the last one banked."""
        G, M = self._auto_groups, self.e.M
        self.e.sync()
        sums = self._auto_sums.download(np.int64, (G, M + 2))
        self._auto_sums.upload(self._auto_zero)     # (after the sync: the next restart_finished adds to zeros)
        if self.dist is not None:
            t = self.to_tensor(sums.reshape(-1))
            self.dist.all_reduce(t)
            sums = np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t, dtype=np.int64).reshape(G, M + 2)
        total = sums[:, :M + 1].sum(axis=0)
        self.score_log.append(total.copy())
        if self.ladder_on:
            self.rung_log.append(sums[:, :M + 1].copy())
        self.length_log.append(sums[:, M + 1].copy())
        self.episode += 1
        self.epsilons.append(self.trainer.epsilon.get())
        if (self.is_learning and self.snapshot_folder is not None and self.snapshot_every
                and self.episode % self.snapshot_every == 0):
            self.snapshots.append(self.trainer.save(id="iteration-%s" % self.episode, overwrite=True,
                                                    folder=self.snapshot_folder))
        return total

    def _episode_end(self):
        if self.auto_reset:
            return self._period_end()
        total = super()._episode_end()
        self.episode += 1
        self.epsilons.append(self.trainer.epsilon.get())
        if self.ladder_on:
            grouped = np.asarray(self.e.episode_scores_grouped(self._groups, self.n_groups), dtype=np.int64)
            if self.dist is not None:
                t = self.to_tensor(grouped.reshape(-1))
                self.dist.all_reduce(t)
                grouped = np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t, dtype=np.int64)
            self.rung_log.append(grouped.reshape(self.n_groups, self.e.M + 1).copy())
        self.e.sync()
        self._seen_done.upload(self._zeros)         # QlearnIA.reset: done = False (:360-368)
        if (self.is_learning and self.snapshot_folder is not None and self.snapshot_every
                and self.episode % self.snapshot_every == 0):
            self.snapshots.append(self.trainer.save(id="iteration-%s" % self.episode, overwrite=True,
                                                    folder=self.snapshot_folder))
        return total

    def _decision(self):
        """lockstep() under action_repeat = K > 1: one decision, held for K lock-steps in one launch."""
        from . import _native as nat
        if self.tick > 0 and self.tick % self.episode_ticks == 0:
            self._episode_end()
        self._play(self.e)
        K, p = self.action_repeat, self.probe
        if p: p("step", True, K)       # K lock-steps go down in this one call
        self.e.step_repeat(self.behaviours, self.seed, self.tick, K, hold_mask_ptr=self._mask.ptr,
                           span_reward_ptr=self._span.ptr, observe=nat.MAP_U8 if self.observe else None)
        if p: p("step", False, K)
        self.tick += K

    def lockstep(self):
        if self.auto_reset:
            self._restart_finished()
        if self.action_repeat > 1:
            self._decision()
        else:
            super().lockstep()
        if (self.checkpoint_every and self.checkpoint_folder is not None and self.tick % self.episode_ticks == 0
                and (self.episode + 1) % self.checkpoint_every == 0):   # this lock-step completed episode number episode + 1
            import os
            os.makedirs(self.checkpoint_folder, exist_ok=True)
            self.checkpoint(os.path.join(self.checkpoint_folder, "checkpoint-latest"))

    def checkpoint(self, path):
        """Write the whole run - arenas, replay memory, trainer, counters - to `path`, between two lock-steps."""
        from . import checkpoint
        return checkpoint.save(self, path)

    def restore(self, path):
        """Continue the run `checkpoint(path)` wrote.  ValueError, with nothing touched, when the checkpoint's dimensions
        or fingerprints differ from this rollout's; returns the checkpoint's manifest."""
        from . import checkpoint
        return checkpoint.load(self, path)

    @property
    def eval_scores(self):
        """Per finished episode: the mean score a policy ship of an evaluation arena banked (empty without eval_arenas)."""
        if not (self.ladder_on and self.eval_arenas):
            return []
        ships = np.flatnonzero(self.policy_mask[0])
        return [float(g[-1][ships].sum()) / float(g[-1][-1] * len(ships)) for g in self.rung_log]

    def _replay(self):
        loss = self.trainer.replay()
        if loss is not None:
            self.losses.append(float(loss[0]) + float(loss[1]))
        return loss

    def _play(self, e):
        """QlearnIA.play for every policy ship (the device keeps each agent's done latch and previous_*)."""
        self.total_steps += 1                      # Agent.step increments before bot_play (agent.py:67-68)
        t, m, lm = self.trainer, self._mask.ptr, self._learn_mask.ptr   # lm is m unless there are evaluation arenas
        collecting = self.total_steps < self.collecting_steps
        replayed = False
        if self.is_learning and self.replay_on_death:
            # obs.done seen for the first time this lock-step (:375-378): counted on the device, one int comes back
            if e.agents_first_done(lm, self._seen_done) > 0:
                self._replay()
                replayed = True
        if self.boltzmann is not None:
            # both heads sampled from softmax(Q / (tau * eps_a)) inside the forward: one call instead of forward + explore
            # (and instead of policy_act); the evaluation arenas stay greedy through their +inf exponent
            e.policy_act_boltzmann(t.weights.ptr, t.epsilon.get(), self.boltzmann[0], self.boltzmann[1], self.seed,
                                   tick=self.capture_tick, collecting=collecting, ship_mask_ptr=m)
            if getattr(t, "actor_priorities", False):
                e.replay_capture_valued(self.capture_tick, ship_mask_ptr=lm)
            else:
                e.replay_capture(self.capture_tick, ship_mask_ptr=lm)
        elif getattr(t, "actor_priorities", False):    # (a duck-typed trainer that predates the option has none)
            # the same choice in one call, with its values; the capture turns them into the new rows' priorities
            e.policy_act(t.weights.ptr, t.epsilon.get(), self.seed, tick=self.capture_tick, collecting=collecting,
                         ship_mask_ptr=m)
            e.replay_capture_valued(self.capture_tick, ship_mask_ptr=lm)
        else:
            e.policy_forward(t.weights.ptr, m)
            e.policy_explore(t.epsilon.get(), self.seed, tick=self.capture_tick, collecting=collecting, ship_mask_ptr=m)
            e.replay_capture(self.capture_tick, ship_mask_ptr=lm)
        e.policy_actions(ship_mask_ptr=m)
        self.capture_tick += 1
        if not collecting and self.is_learning:
            t.decay_epsilon()
        # at most ONE replay per lock-step: the batched replay already draws from every arena's memory, a second one on
        # the same lock-step (deaths AND total_steps % 50 == 0) would fit the same memories twice
        if self.is_learning and self.replay_every and self.total_steps % self.replay_every == 0 and not replayed:
            self._replay()
