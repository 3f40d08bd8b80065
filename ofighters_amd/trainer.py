"""DeviceTrainer - the batched, device-resident counterpart of the reference's `Trainer` (agents/qlearnIA_V2.py:46-298)
for an ArenaBatch: weights, Adam state and the replay memory live in HBM; `get_best_action` is
ArenaBatch.policy_forward + policy_explore, `remember` is ArenaBatch.replay_capture, and `replay(batch_size)`
(:240-285) is sample -> gather -> targets -> one fit step - one draw (`_draw_window` or, under global_sampling,
`_draw_list`) that `_fit` consumes, whatever the options below -, all through the C-ABI (ofx_replay_sample, ofx_replay_gather,
ofx_dqn_targets, ofx_dqn_fit - or ofx_dqn_fit_reference with `reference_quirks=True`: the reference's step as written,
ptr_target[x][y] and the fit on next_state's inputs included, :280-283).

`prioritized=True` (opt-in, not in the reference) turns on proportional prioritized experience replay (Schaul et al.
2016): ofx_replay_sample_prioritized draws the minibatch by priority, ofx_dqn_fit_weighted takes the window's
importance-sampling weights (beta annealed linearly from per_beta to 1 over per_beta_steps fit steps) and returns the
rows' TD errors, which ofx_replay_update_priorities writes back.

`n_step=n` (opt-in, not in the reference; 1 = the one-step targets above) bootstraps every target n lock-steps ahead:
ofx_replay_gather_nstep follows each sampled row's ship through its following rows (until n rows, its death, an episode
restart or the newest row), gathers the chain's last next-state maps and the discounted return ret = sum gamma^k r_k with
the discount disc = gamma^L (0 after a death), and ofx_dqn_targets_nstep forms y = ret + disc * max(next_state).  Works
with `prioritized` (the priorities become n-step TD errors); the return is not corrected for the off-policy actions
inside the chain (as in Rainbow).

`target_sync=K` or `target_tau=tau` (opt-in, not in the reference; one of them) keeps a target network: a second device
blob that starts as a copy of the initial weights and that the targets bootstrap from instead of the blob being fitted.
After every fit step ofx_policy_blend_weights moves it: a hard copy of the online weights after every K-th step
(fit_steps % K == 0), or target = (1 - tau) * target + tau * online after each one.  `double_dqn=True` forms the targets
with ofx_dqn_targets_double (van Hasselt et al. 2016): the online blob selects the next action and pointer, the target
blob evaluates them (without a target network both are the online blob, which gives the plain targets).  All of it works
with `prioritized` and `n_step`; the fit's current values and TD errors always come from the online blob, and save()
stores the online blob only.

`huber_delta=d` and `clip_norm=c` (opt-in, not in the reference; each None or a finite value > 0) bound how an error
becomes a weight update, the fit step going through ofx_dqn_fit_robust under every sampler.  huber_delta replaces the
squared error of both heads by Keras's Huber(d) (Mnih et al. 2015's error clip): quadratic up to |e| = d, linear beyond,
so a row's seed is clamp(e, -d, d) - inside the quadratic zone HALF the mse gradient, as in Keras - while the
priorities of `prioritized` stay the raw |TD error|.  clip_norm scales the whole gradient by
min(1, c / (norm + 1e-6)) before Adam (torch.nn.utils.clip_grad_norm_).  With either set, `grad_norms` collects the
gradient's norm before clipping of every fit step, next to `losses` (which then holds the Huber losses).  Both work with
`prioritized`, `n_step`, the target network and `double_dqn`, which only change targets and sampling.

`packed_memory=True` (opt-in, exact) builds the replay memory with ArenaBatch.replay_create(packed=True): the stored
observation maps are kept as the pairs of their nonzero words in a pool of `memory_pool_pairs` pairs per arena (0 = the
library's default, about a tenth of the dense ring's HBM) instead of the dense frame ring, which is what lets a trainer
exist at 32 768 arenas on one card.  Sampling, gathering, targets and the fit see the same bytes, so a run fits the same
bits as with the dense ring as long as no arena's pool overflows (batch.replay_store_stats()["evicted"] == 0); a pool that
is too small releases the oldest frames early and their rows stop being sampled.  memory_pool_pairs must be an integer
>= 0 (no bool) and 0 without packed_memory: ValueError before anything is allocated.  Neither argument enters
fingerprint() or a checkpoint's manifest: a checkpoint is form-agnostic (the blob carries frame_tick, early evictions
included), a run restored under the same memory_pool_pairs continues bit for bit, and restoring into a pool that cannot
hold the blob's frames is refused by the import.

`global_sampling=True` (opt-in, not in the reference) draws ONE minibatch of `fit_batch` rows per replay from the union of
all arenas' memories instead of `batch_size` rows in every arena of which a moving window of fit_batch is fitted:
ofx_replay_sample_global picks the rows uniformly over rows or, with `prioritized`, proportionally to their priorities
across arenas (the IS weights then correct to uniform over rows and arrive max-normalised), ofx_replay_gather_list
materialises exactly those rows and ofx_replay_update_priorities_list writes the TD errors back and levels every arena's
running maximum to the global one.  replay() then costs no [N]-sized download and fits min(fit_batch, eligible rows);
`batch_size` is unused.  Works with `prioritized`, `n_step`, the target network, `double_dqn`, `huber_delta`, `clip_norm`
and `packed_memory`; refused with reference_quirks (ValueError); the value must be a bool.  fingerprint() carries
"global_sampling": True only when it is on, so a state taken under one sampler is refused under the other, and `draws`
keys the sampler's Philox stream as before: a checkpoint needs nothing new.

`accumulate=k` (opt-in, not in the reference; an integer >= 1 and no bool, 1 = off; k > 1 needs global_sampling and is
refused with reference_quirks: ValueError naming accumulate before anything is allocated) makes one fit step out of k
micro-batches: replay() draws k * fit_batch rows in ONE ofx_replay_sample_global call (with `prioritized` the IS weights
are max-normalised over the whole draw), cuts the n rows drawn into c = max(1, n // fit_batch) chunks of fit_batch rows
(one chunk of n rows while n < fit_batch; rows beyond c * fit_batch are not fitted), and runs gather, targets and
ofx_dqn_grad per chunk - the chunks are pointer offsets into the draw's sorted list - summing gradient, batch statistics
and losses into one device accumulator; one ofx_dqn_apply then applies their mean (scale = 1 / c; clip_norm acts on
that mean), the priorities of all fitted rows are written back and the target network moves.  The fit's workspace is
that of ONE chunk, which is the point: the step's batch is no longer bounded by it.  BatchNorm normalises every chunk by
its own batch statistics and the moving statistics take their mean, so k chunks are not bit for bit one fit of k *
fit_batch rows.  One replay is still one draw and one fit step.  `grad_hook` (an attribute, None by default) is called as
hook(trainer, acc_buffer) between the last ofx_dqn_grad and ofx_dqn_apply with the accumulator's DeviceBuffer
(batch.dqn_acc_floats() floats: include/ofx.h) and returns how many accumulators it summed into the buffer (None or 1: it
is untouched); the scale becomes 1 / (c * that count).  It is the place for a data-parallel caller's SUM all-reduce.  With
a hook set the step goes through ofx_dqn_grad + ofx_dqn_apply also at accumulate=1 (one chunk: the fused step's bits)
under every sampler of the textbook fit.  fingerprint() carries "accumulate": k only when k > 1; the accumulator is scratch inside
one replay(), so a checkpoint needs nothing new.

`actor_priorities=True` (opt-in, not in the reference; Horgan et al. 2018, Ape-X; needs `prioritized`, refused with
reference_quirks, the value must be a bool: ValueError naming actor_priorities before anything is allocated) gives every
new row the priority of the TD error the actor can form itself instead of the arena's running maximum.  At training sizes
(thousands of arenas, one replay per lock-step at the most) nearly every row leaves the memory without ever being fitted,
so under the running-maximum rule the sampler draws almost uniformly over rows that all carry the same mass.
TrainingRollout then plays through ofx_policy_act, which returns Q(s, a) and the heat map's value at the chosen pointer
next to both heads' maxima, and captures through ofx_replay_capture_valued, which forms the two errors of a row the
moment its next state is seen.  Three things to know: the initial priority is the ONE-STEP error, also with n_step > 1;
it is formed with the ONLINE blob in inference mode - a target network and double_dqn do not enter; and the first
write-back replaces it with the learner's error, as before.  The actions played and the rows stored do not change.
fingerprint() carries "actor_priorities": True only when it is on; a checkpoint gains the section
`replay_actor_values` (the ships' previous values), the replay blob keeps its format.

`soft_targets=(tau_act, tau_ptr)` and `munchausen=(alpha, clip)` (opt-in, not in the reference; each None or a pair of
finite floats: ValueError naming the argument before anything is allocated) change what the targets bootstrap from, through
ofx_dqn_targets_soft.  soft_targets replaces the hard maximum of next_state by the soft (entropy-regularised) value of
soft Q-learning, V_T = T ln sum_a exp(Q(a) / T) - over the two actions at tau_act, over the heat map's 160 000 pixels at
tau_ptr, reduced inside the streaming head kernel; each tau is 0 (that head keeps its maximum) or lies in [1e-6, 1e30].
It is the backup that matches a Boltzmann behaviour policy (TrainingRollout(boltzmann=...)), and (0.0, 0.0) fits the
default trainer's bits.  munchausen (Vieillard et al. 2020; alpha in [0, 1], clip finite and <= 0) adds alpha * clamp(Q(s, a)
- V_T(s), clip, 0) - the scaled, clipped log-policy of the action taken - to the reward of both heads, from one more
forward on `state`; it needs soft_targets with both taus > 0 and n_step == 1.  Both are refused with double_dqn (a soft
backup has no selection step) and with reference_quirks, and work with `prioritized`, a target network (the soft values
and Munchausen's log-policy then come from the target blob), n_step (soft only), huber_delta / clip_norm, packed_memory,
global_sampling, accumulate and actor_priorities - whose initial priority stays the HARD one-step error the actor
forms from the maxima it plays with.  fingerprint() carries "soft_targets" / "munchausen" only when set; a
checkpoint needs nothing new.

`augment="flips"`, `"d4"` or an integer mask in 1..255 (opt-in, not in the reference; no bool; anything else: ValueError
naming augment before anything is allocated; refused with reference_quirks) augments every gathered chunk by the
symmetries of the square arena (RAD, Laskin et al. 2020; DrQ, Kostrikov et al. 2020): right after a chunk's gather,
ofx_replay_augment draws one of the allowed isometries per row - bit g of the mask allows element g of include/ofx.h's
"symmetry augmentation"; "flips" = 0x55 is the identity, the two mirrors and the half turn, "d4" = 0xFF all eight - and
applies it in place to the row's two observations: both 1-bit maps of state and next_state, the pointing and position
elements of both heads, and the stored pointer.  It is the row COPIES in `rows` that are transformed, never the memory:
targets of every flavour, the fit in both forms and ofx_dqn_grad read only (rows, bits_prev, bits_next) and so see one
consistent transformed transition - munchausen's probe reads the transformed pointer -, and the priority write-back
still finds its ring rows through (tick_prev, ship), which the copies keep.  The element of a row is a pure function of
(seed, the replay's draw counter, the row's position in the draw), so chunks of one draw do not repeat each other's
operations and a checkpoint needs nothing new.  Works with every other option of the textbook fit; how symmetric the
game itself is under each element is measured in DESIGN.md.  fingerprint() carries "augment": mask only when set.

save() and a checkpoint are different things.  save() writes the online blob alone as the Keras-compatible `.npz`
(`model.get_weights()` order): something to load into a model and play with; a run "resumed" from it starts over with a
cold optimiser, an empty memory and epsilon at its start.  state_dict() / load_state_dict() carry what the trainer itself
needs to go on as if it had never stopped - weights, both Adam moments, the target blob, the fit / draw counters that key
the sampler's Philox streams and the Adam bias correction, the loss lists and the epsilon schedule's position - guarded by
a fingerprint of the hyperparameters that must match.  TrainingRollout.checkpoint() adds the replay memory, the arenas
and its own counters (ofighters_amd/checkpoint.py); a run restored from it continues bit for bit."""
import numpy as np

from .engine import DeviceBuffer, check_pool_pairs
from .lib.epsilon import Epsilon_cos


def epsilon_state(eps):
    """An exploration schedule's position: its class name and scalar attributes (lib/epsilon.py keeps the reference's
    API, so the state is read and set from here)."""
    return {"class": type(eps).__name__,
            "attrs": {k: v for k, v in sorted(vars(eps).items())
                      if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)}}


def set_epsilon_state(eps, state):
    if type(eps).__name__ != state["class"]:
        raise ValueError("epsilon schedule: the state is a %s's, the trainer has a %s" % (state["class"], type(eps).__name__))
    for k, v in state["attrs"].items():
        setattr(eps, k, v.item() if isinstance(v, np.generic) else v)


def fingerprint_diff(have, want):
    """The keys on which two fingerprints differ (missing keys included), sorted."""
    return sorted(k for k in set(have) | set(want) if k not in have or k not in want or have[k] != want[k])


AUGMENT_MASKS = {"flips": 0x55, "d4": 0xFF}                  # identity, both mirrors, half turn / the whole dihedral group


def _augment_mask(val):
    """None, or the element mask of `augment`: a name of AUGMENT_MASKS or an integer in 1..255 (no bool)."""
    if val is None:
        return None
    if isinstance(val, str) and val in AUGMENT_MASKS:
        return AUGMENT_MASKS[val]
    if isinstance(val, (int, np.integer)) and not isinstance(val, (bool, np.bool_)) and 1 <= val <= 255:
        return int(val)
    raise ValueError("DeviceTrainer: augment must be None, %s or an integer mask in 1..255, got %r"
                     % (", ".join(repr(k) for k in AUGMENT_MASKS), val))


def _float_pair(name, val):
    """None, or `val` as a tuple of two finite floats (no bools); ValueError naming the argument otherwise."""
    if val is None:
        return None
    try:
        pair = tuple(val)
        ok = len(pair) == 2 and all(isinstance(x, (int, float, np.integer, np.floating)) and
                                    not isinstance(x, (bool, np.bool_)) for x in pair)
        pair = tuple(float(x) for x in pair) if ok else None
    except (TypeError, ValueError):
        pair = None
    if pair is None or not all(np.isfinite(x) for x in pair):
        raise ValueError("DeviceTrainer: %s must be None or a pair of finite floats, got %r" % (name, val))
    return pair


class _At:
    """A position inside a DeviceBuffer for the engine calls that take one (they read .ptr alone); owns nothing."""

    def __init__(self, buf, offset):
        self.ptr = buf.ptr + int(offset)


class DeviceTrainer:
    global_sampling = False                                  # the opt-in of __init__; off on any trainer that never set it
    accumulate = 1                                           # likewise: micro-batches per fit step
    actor_priorities = False                                 # likewise: new rows enter at the actor's own TD error
    grad_hook = None                                         # hook(trainer, acc_buffer) before ofx_dqn_apply; see above
    soft_targets = None                                      # likewise: (tau_act, tau_ptr) of the soft backup
    munchausen = None                                        # likewise: (alpha, clip) of the Munchausen term
    augment = None                                           # likewise: the element mask of the symmetry augmentation

    def __init__(self, batch, weights, learning_rate=0.0001, epsilon=None, batch_size=8, memory_size=400, frames=0,
                 seed=0x0F160003, fit_batch=256, reference_quirks=False, prioritized=False, per_alpha=0.6, per_beta=0.4,
                 per_beta_steps=50_000, per_eps=1e-3, n_step=1, target_sync=0, target_tau=None, double_dqn=False,
                 huber_delta=None, clip_norm=None, packed_memory=False, memory_pool_pairs=0, global_sampling=False,
                 accumulate=1, actor_priorities=False, soft_targets=None, munchausen=None, augment=None):
        augment = _augment_mask(augment)
        if augment is not None and reference_quirks:
            raise ValueError("DeviceTrainer: augment needs the textbook fit (reference_quirks=False is the reference's "
                             "replay on its own memory as written)")
        soft_targets = _float_pair("soft_targets", soft_targets)
        munchausen = _float_pair("munchausen", munchausen)
        if soft_targets is not None:
            for tau in soft_targets:
                if not (tau == 0.0 or 1e-6 <= tau <= 1e30):
                    raise ValueError("DeviceTrainer: soft_targets takes (tau_act, tau_ptr), each 0 or in [1e-6, 1e30], got %r"
                                     % (soft_targets,))
        if munchausen is not None:
            if not (0.0 <= munchausen[0] <= 1.0 and munchausen[1] <= 0.0):
                raise ValueError("DeviceTrainer: munchausen takes (alpha, clip) with alpha in [0, 1] and clip <= 0, got %r"
                                 % (munchausen,))
            if soft_targets is None or not (soft_targets[0] > 0.0 and soft_targets[1] > 0.0):
                raise ValueError("DeviceTrainer: munchausen needs soft_targets with both taus > 0 (its log-policy is the "
                                 "softmax's), got soft_targets=%r" % (soft_targets,))
            if n_step != 1:
                raise ValueError("DeviceTrainer: munchausen needs n_step == 1 (the term belongs to one action's reward)")
        for name, val in (("soft_targets", soft_targets), ("munchausen", munchausen)):
            if val is not None and double_dqn:
                raise ValueError("DeviceTrainer: %s is refused with double_dqn (a soft backup has no selection step)" % name)
            if val is not None and reference_quirks:
                raise ValueError("DeviceTrainer: %s needs the textbook fit (reference_quirks=False computes its own "
                                 "targets)" % name)
        memory_pool_pairs = check_pool_pairs("DeviceTrainer: memory_pool_pairs", packed_memory, memory_pool_pairs)
        if not isinstance(actor_priorities, (bool, np.bool_)):
            raise ValueError("DeviceTrainer: actor_priorities must be a bool, got %r" % (actor_priorities,))
        if actor_priorities and not prioritized:
            raise ValueError("DeviceTrainer: actor_priorities needs prioritized=True (it sets the priority a new row "
                             "enters the memory with)")
        if actor_priorities and reference_quirks:
            raise ValueError("DeviceTrainer: actor_priorities needs the textbook fit (reference_quirks=False)")
        if not isinstance(global_sampling, (bool, np.bool_)):
            raise ValueError("DeviceTrainer: global_sampling must be a bool, got %r" % (global_sampling,))
        if isinstance(accumulate, (bool, np.bool_)) or not isinstance(accumulate, (int, np.integer)) or accumulate < 1:
            raise ValueError("DeviceTrainer: accumulate must be an integer >= 1, got %r" % (accumulate,))
        if accumulate > 1 and reference_quirks:
            raise ValueError("DeviceTrainer: accumulate > 1 needs the textbook fit (reference_quirks=False is the "
                             "reference's one fit per replay as written)")
        if accumulate > 1 and not global_sampling:
            raise ValueError("DeviceTrainer: accumulate > 1 needs global_sampling=True (the k * fit_batch rows of a step "
                             "are one draw from all arenas' memories)")
        if global_sampling and reference_quirks:
            raise ValueError("DeviceTrainer: global sampling needs the textbook fit (reference_quirks=False is the "
                             "reference's replay over its own memory as written)")
        if prioritized and reference_quirks:
            raise ValueError("DeviceTrainer: prioritized replay needs the textbook fit (reference_quirks=False)")
        if int(n_step) != n_step or n_step < 1:
            raise ValueError("DeviceTrainer: n_step must be an integer >= 1, got %r" % (n_step,))
        if n_step > 1 and reference_quirks:
            raise ValueError("DeviceTrainer: n-step returns need the textbook fit (reference_quirks=False computes its own "
                             "one-step targets)")
        if isinstance(target_sync, bool) or not isinstance(target_sync, (int, np.integer)) or target_sync < 0:
            raise ValueError("DeviceTrainer: target_sync must be an integer >= 0, got %r" % (target_sync,))
        if target_tau is not None and not (0.0 < float(target_tau) <= 1.0):      # NaN fails the comparison
            raise ValueError("DeviceTrainer: target_tau must lie in (0, 1], got %r" % (target_tau,))
        if target_sync and target_tau is not None:
            raise ValueError("DeviceTrainer: give target_sync (hard copies) or target_tau (soft updates), not both")
        if (target_sync or target_tau is not None or double_dqn) and reference_quirks:
            raise ValueError("DeviceTrainer: a target network / Double DQN needs the textbook fit (reference_quirks=False "
                             "computes its own targets)")
        for name, val in (("huber_delta", huber_delta), ("clip_norm", clip_norm)):
            if val is None:
                continue
            if isinstance(val, bool) or not (0.0 < float(val) < float("inf")):       # NaN fails the comparison
                raise ValueError("DeviceTrainer: %s must be None or a finite value > 0, got %r" % (name, val))
            if reference_quirks:
                raise ValueError("DeviceTrainer: %s needs the textbook fit (reference_quirks=False is the reference's "
                                 "mse into plain Adam as written)" % name)
        self.batch = batch                                  # the ArenaBatch this trainer plays and learns on
        w = np.ascontiguousarray(weights, np.float32)
        self.n_floats = w.size
        self.weights = DeviceBuffer(w.nbytes).upload(w)
        zeros = np.zeros_like(w)
        self.adam_m = DeviceBuffer(w.nbytes).upload(zeros)
        self.adam_v = DeviceBuffer(w.nbytes).upload(zeros)
        self.target_sync = int(target_sync)                 # K > 0: target <- online after every K-th fit step
        self.target_tau = None if target_tau is None else float(target_tau)   # target <- (1 - tau) target + tau online
        self.double_dqn = bool(double_dqn)                  # select with the online blob, evaluate with the target blob
        # the target network: a device copy of the initial weights, or None (the targets bootstrap from self.weights)
        self.target = DeviceBuffer(w.nbytes).upload(w) if (self.target_sync or self.target_tau is not None) else None
        self.learning_rate = learning_rate                  # lr = 0.0001 (qlearnIA_V2.py:306)
        self.gamma = 0.9                                    # :51
        self.epsilon = epsilon if epsilon is not None else Epsilon_cos(period=110 * 400)
        self.batch_size = batch_size                        # 8 (:307)
        self.seed = seed
        self.fit_batch = fit_batch                          # rows per optimisation step (the reference fits on 8): one
                                                            # replay takes 3.6 ms at 64 rows, 5.8 at 256 - about one
                                                            # lock-step of a 4096-arena batch -, 42 ms at 4096
        self.reference_quirks = bool(reference_quirks)      # Trainer.replay as written instead of the textbook DQN step
        self.prioritized = bool(prioritized)                # PER: priority exponent alpha, IS exponent beta -> 1, eps
        self.per_alpha, self.per_beta, self.per_beta_steps, self.per_eps = per_alpha, per_beta, per_beta_steps, per_eps
        self.n_step = int(n_step)                           # TD targets bootstrap n_step lock-steps ahead (1: one-step)
        self.huber_delta = None if huber_delta is None else float(huber_delta)   # Huber(delta) in place of the mse
        self.clip_norm = None if clip_norm is None else float(clip_norm)         # global gradient-norm clip before Adam
        self.fit_steps = 0
        self.draws = 0
        self.losses = []
        self.grad_norms = []                                 # with huber_delta / clip_norm: every fit step's pre-clip norm
        self._buf = {}                                       # replay scratch kept between calls (grow-only)
        self.packed_memory = bool(packed_memory)             # the replay memory's frame store: packed pairs or dense ring
        self.memory_pool_pairs = memory_pool_pairs           # pairs per arena of the packed store (0: the library's default)
        self.global_sampling = bool(global_sampling)         # one minibatch of fit_batch rows from all arenas' memories
        self.accumulate = int(accumulate)                    # micro-batches of fit_batch rows per fit step
        self.actor_priorities = bool(actor_priorities)       # a new row's mass: the actor's one-step TD error
        self.soft_targets = soft_targets                     # (tau_act, tau_ptr): soft values in place of the maxima
        self.munchausen = munchausen                         # (alpha, clip): the clipped log-policy joins the reward
        self.augment = augment                               # mask of the isometries a gathered row may be seen under
        if self.packed_memory:
            batch.replay_create(memory_size, frames, packed=True, pool_pairs=memory_pool_pairs)
        else:
            batch.replay_create(memory_size, frames)
        if self.prioritized:
            batch.replay_prioritize(per_alpha, per_eps)
        if self.actor_priorities:
            batch.replay_actor_priorities(self.gamma)

    def _scratch(self, name, nbytes):
        """A device buffer of at least nbytes that lives as long as the trainer: no hipMalloc / hipFree per replay."""
        b = self._buf.get(name)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                self.batch.sync()
                b.free()
            b = self._buf[name] = DeviceBuffer(int(nbytes))
        return b

    def decay_epsilon(self):
        self.epsilon.next()

    def weights_host(self):
        self.batch.sync()
        return self.weights.download(np.float32, (self.n_floats,))

    def target_host(self):
        """The target network's blob like weights_host(), or None without a target network."""
        if self.target is None:
            return None
        self.batch.sync()
        return self.target.download(np.float32, (self.n_floats,))

    def save(self, id=None, overwrite=False, folder="networks", name="bi_head_pointer"):
        """Trainer.save (qlearnIA_V2.py:289-298): `keras-model-<name>[-<id>]` under the networks folder, as the .npz
        of `model.get_weights()` (agents/policy_weights.py) that the facade's Trainer.load and a Keras
        `model.set_weights(list(np.load(f).values()))` read back."""
        import os
        from .agents.policy_weights import save_npz
        fname = "keras-model-" + name + ("-" + str(id) if id else "") + ".npz"
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, fname)
        if os.path.exists(path) and not overwrite:
            raise Exception("%s exists (overwrite=False)" % path)
        save_npz(path, self.weights_host())
        return path

    def fingerprint(self):
        """The hyperparameters a state must have been taken under to be loaded here."""
        b = self.batch
        fp = {"n_floats": int(self.n_floats), "learning_rate": float(self.learning_rate), "gamma": float(self.gamma),
              "batch_size": int(self.batch_size), "fit_batch": int(self.fit_batch), "seed": int(self.seed),
                "reference_quirks": self.reference_quirks, "prioritized": self.prioritized,
                "per_alpha": float(self.per_alpha), "per_beta": float(self.per_beta),
                "per_beta_steps": int(self.per_beta_steps), "per_eps": float(self.per_eps), "n_step": self.n_step,
                "target_sync": self.target_sync, "target_tau": self.target_tau, "double_dqn": self.double_dqn,
                "huber_delta": self.huber_delta, "clip_norm": self.clip_norm,
                "memory_capacity": int(b.replay_capacity), "memory_frames": int(b.replay_frames)}
        if self.global_sampling:                             # only when on: a default trainer's key set stays as it was,
            fp["global_sampling"] = True                     # and fingerprint_diff counts the missing key as a difference
        if self.accumulate > 1:                              # the same pattern
            fp["accumulate"] = self.accumulate
        if self.actor_priorities:
            fp["actor_priorities"] = True
        if self.soft_targets is not None:
            fp["soft_targets"] = list(self.soft_targets)
        if self.munchausen is not None:
            fp["munchausen"] = list(self.munchausen)
        if self.augment is not None:
            fp["augment"] = self.augment
        return fp

    def state_dict(self):
        """Everything of the trainer that a resumed run needs (host copies; the replay memory belongs to the batch)."""
        self.batch.sync()
        blob = lambda buf: buf.download(np.float32, (self.n_floats,))
        return {"fingerprint": self.fingerprint(), "weights": blob(self.weights), "adam_m": blob(self.adam_m),
                "adam_v": blob(self.adam_v), "target": None if self.target is None else blob(self.target),
                "fit_steps": int(self.fit_steps), "draws": int(self.draws),
                "losses": np.array(self.losses, np.float64).reshape(-1, 2), "grad_norms": np.array(self.grad_norms, np.float64),
                "epsilon": epsilon_state(self.epsilon)}

    def load_state_dict(self, d):
        """Take over a state_dict().  The fingerprint is compared first: any difference raises ValueError listing every
        differing key before a device write.  The blobs go into the existing device buffers, so pointers held elsewhere
        (a pinned policy) stay valid; pin the weights again to have them prepared."""
        diff = fingerprint_diff(self.fingerprint(), d["fingerprint"])
        if diff:
            raise ValueError("DeviceTrainer.load_state_dict: the state was taken under other hyperparameters: "
                             + ", ".join("%s (%r here, %r there)" % (k, self.fingerprint().get(k), d["fingerprint"].get(k))
                                         for k in diff))
        blobs = {}
        for k in ("weights", "adam_m", "adam_v", "target"):
            if k == "target" and self.target is None:
                if d.get("target") is not None:
                    raise ValueError("DeviceTrainer.load_state_dict: the state has a target network, this trainer none")
                continue
            a = d.get(k)
            if a is None or np.asarray(a).dtype != np.float32 or np.asarray(a).shape != (self.n_floats,):
                raise ValueError("DeviceTrainer.load_state_dict: %s must be float32 [%d]" % (k, self.n_floats))
            blobs[k] = np.ascontiguousarray(a)
        if type(self.epsilon).__name__ != d["epsilon"]["class"]:
            set_epsilon_state(self.epsilon, d["epsilon"])       # raises
        self.batch.sync()
        for k, a in blobs.items():
            getattr(self, k).upload(a)
        self.fit_steps, self.draws = int(d["fit_steps"]), int(d["draws"])
        self.losses = [(float(a), float(b)) for a, b in np.asarray(d["losses"], np.float64).reshape(-1, 2)]
        self.grad_norms = [float(x) for x in np.asarray(d["grad_norms"], np.float64).reshape(-1)]
        set_epsilon_state(self.epsilon, d["epsilon"])

    def replay(self, batch_size=None):
        """One Trainer.replay: draw a minibatch - min(batch_size, len(memory)) rows per arena of which a moving window is
        fitted, or under global_sampling one list of rows from all arenas' memories -, then targets and one fit step on it.
        Returns (mse(output1), mse(output2)) or None while there is nothing to fit."""
        draw = self._draw_list() if self.global_sampling else self._draw_window(int(batch_size or self.batch_size))
        return None if draw is None else self._fit(*draw)

    # A draw is (n, gather, row_w, write_back): n rows to fit; gather(o, m, rows, bits_prev, bits_next, ret, disc)
    # materialises rows o .. o + m - 1 of them (ret / disc None: one-step) and, where the weights are per window, fills
    # row_w; row_w the rows' IS weights (None without PER); write_back(k, rows_ptr, td_ptr) the first k rows' priorities.
    def _draw_window(self, bs):
        """The default sampler: bs rows per arena, of which a window of fit_batch that moves with the draw counter is
        fitted; under PER drawn by priority and weighted by the window's max-normalised IS weights."""
        b = self.batch
        cnt, _ = b.replay_count()
        if int(cnt.max()) == 0:
            return None
        per = self.prioritized
        slot, n_s = self._scratch("slot", 4 * b.N * bs), self._scratch("n_s", 4 * b.N)
        if per:
            isw = self._scratch("is_w", 4 * b.N * bs)
            b.replay_sample_prioritized(self.seed, self.draws, bs, self.beta(), slot, n_s, isw)
        else:
            b.replay_sample(self.seed, self.draws, bs, slot, n_s)
        self.draws += 1
        # the sampled transitions of all arenas, WITHOUT the -1 pads of arenas that hold fewer than bs (a pad would enter
        # the BatchNorm batch statistics and the loss scale of the fit; the reference's batch is min(bs, len(memory)) real
        # rows); one optimisation step takes a window of them that moves with the draw counter
        # n_sampled, not min(len, bs): a row whose `state` frame has left the arena's frame ring is not sampled
        b.sync()
        n_valid = int(n_s.download(np.int32, (b.N,)).sum())
        if n_valid == 0:
            return None
        n = min(n_valid, int(self.fit_batch))                # at most fit_batch: a window is always one chunk
        start = ((self.draws - 1) * n) % (n_valid - n + 1)
        row_w = self._scratch("row_w", 4 * n) if per else None

        def gather(o, m, rows, bits_prev, bits_next, ret, disc):
            if ret is None:
                got = b.replay_gather_valid_into(slot, n_s, bs, start, m, rows, bits_prev, bits_next)
            else:
                got = b.replay_gather_nstep_into(slot, n_s, bs, start, m, self.n_step, self.gamma, rows, bits_prev,
                                                 bits_next, ret, disc)
            if got != m:
                raise Exception("DeviceTrainer.replay: gathered %d of %d rows" % (got, m))
            if per:
                b.replay_window_weights_into(isw, n_s, bs, start, m, row_w)

        return n, gather, row_w, lambda k, rows_p, td_p: b.replay_update_priorities(slot, n_s, bs, start, k, rows_p, td_p)

    def _draw_list(self):
        """global_sampling: accumulate * fit_batch rows in one draw from the union of all arenas' memories (uniform over
        rows, or by priority across arenas); a chunk is a pointer offset into the draw's sorted list.  The sampler's two
        host integers are the only synchronisation before the fit."""
        b = self.batch
        nb = self.accumulate * int(self.fit_batch)
        per = self.prioritized
        arena, slot, row_w, n, _ = b.replay_sample_global(self.seed, self.draws, nb, per, self.beta() if per else 0.0,
                                                          self._scratch("g_arena", 4 * nb), self._scratch("g_slot", 4 * nb),
                                                          self._scratch("row_w", 4 * nb) if per else None)
        self.draws += 1
        if n == 0:
            return None

        def gather(o, m, rows, bits_prev, bits_next, ret, disc):
            nstep = () if ret is None else (self.n_step, self.gamma, ret, disc)
            b.replay_gather_list_into(_At(arena, 4 * o), _At(slot, 4 * o), m, rows, bits_prev, bits_next, *nstep)

        return n, gather, row_w, lambda k, rows_p, td_p: b.replay_update_priorities_list(arena, slot, k, rows_p, td_p)

    def _fit(self, n, gather, row_w, write_back):
        """One fit step on a draw of n rows, cut into c = max(1, n // fit_batch) chunks of fit_batch rows (one chunk of
        all n rows while n < fit_batch; rows beyond c * fit_batch are drawn but NOT fitted): gather and targets per
        chunk, then the fused fit - or, with accumulate > 1 or a grad_hook, ofx_dqn_grad per chunk, the hook and one
        ofx_dqn_apply with scale = 1 / (c * the hook's count) -, the write-back over all fitted rows and the target
        network's move.  `rows` holds every chunk (the write-back reads them); the maps, targets and returns one chunk.
        The step is counted before the first gather, so a window gather that raises leaves fit_steps one higher."""
        b = self.batch
        fb = int(self.fit_batch)
        c = max(1, n // fb)
        m = fb if n >= fb else n                             # rows per chunk
        per = self.prioritized
        quirks = self.reference_quirks                       # (window draws only) the reference's own targets and fit
        split = (self.accumulate > 1 or self.grad_hook is not None) and not quirks
        words = b.W * b.H // 32
        row_bytes = b.TRANSITION_DTYPE.itemsize
        rows = self._scratch("rows", c * m * row_bytes)
        bits_prev, bits_next = self._scratch("bits_prev", 4 * m * 2 * words), self._scratch("bits_next", 4 * m * 2 * words)
        ret, disc = (self._scratch("ret", 4 * m), self._scratch("disc", 4 * m)) if self.n_step > 1 else (None, None)
        if not quirks:
            y_act, y_ptr = self._scratch("y_act", 4 * m), self._scratch("y_ptr", 4 * m)
        td = self._scratch("td", 8 * c * m) if per else None
        acc = self._scratch("acc", 4 * b.dqn_acc_floats()) if split else None
        self.fit_steps += 1
        for i in range(c):
            o = i * m
            rows_i = _At(rows, o * row_bytes)
            gather(o, m, rows_i, bits_prev, bits_next, ret, disc)
            if self.augment is not None:                     # this replay's draw has already been counted
                b.replay_augment_into(self.seed, self.draws - 1, o, m, self.augment, rows_i, bits_prev, bits_next)
            if quirks:                                       # as written: no hook, no split, its targets inside the fit
                loss = b.dqn_fit_reference(self.weights, self.adam_m, self.adam_v, self.fit_steps, self.learning_rate, m,
                                           rows_i.ptr, bits_prev.ptr, bits_next.ptr, self.gamma)
                continue
            self._targets(m, rows_i.ptr, bits_prev.ptr, bits_next.ptr, y_act, y_ptr)
            chunk = (m, rows_i.ptr, bits_prev.ptr, y_act.ptr, y_ptr.ptr)
            w_p, td_p = (row_w.ptr + 4 * o, td.ptr + 8 * o) if per else (None, None)
            if split:
                b.dqn_grad(self.weights, *chunk, acc, i == 0, self.huber_delta or 0.0, w_p, td_p)
            else:
                loss = self._fit_fused(*chunk, w_p, td_p)
        if split:
            loss = self._apply(acc, c)
        if per:
            write_back(c * m, rows.ptr, td.ptr)
        self._move_target()
        self.losses.append(loss)
        return loss

    def _fit_fused(self, m, rows_p, prev_p, y_act_p, y_ptr_p, w_p, td_p):
        """The fit step in one call: ofx_dqn_fit_robust with huber_delta / clip_norm (the pre-clip gradient norm goes to
        grad_norms), else ofx_dqn_fit_weighted under PER, else ofx_dqn_fit."""
        b = self.batch
        step = (self.weights, self.adam_m, self.adam_v, self.fit_steps, self.learning_rate, m, rows_p, prev_p, y_act_p, y_ptr_p)
        if self._robust():
            l1, l2, norm = b.dqn_fit_robust(*step, self.huber_delta or 0.0, self.clip_norm or 0.0, w_p, td_p)
            self.grad_norms.append(norm)
            return l1, l2
        if self.prioritized:
            return b.dqn_fit_weighted(*step, w_p, td_p)
        return b.dqn_fit(*step)

    def _apply(self, acc, chunks):
        """The hook, then ofx_dqn_apply on the mean of `chunks` x (the hook's count) accumulated micro-batches; the norm
        before clipping goes to grad_norms where the fused step reports it (huber_delta / clip_norm)."""
        count = self.grad_hook(self, acc) if self.grad_hook is not None else None
        count = 1 if count is None else count
        if isinstance(count, bool) or int(count) != count or count < 1:
            raise ValueError("DeviceTrainer: grad_hook must return None or the integer count >= 1 of accumulators it "
                             "summed, got %r" % (count,))
        l1, l2, norm = self.batch.dqn_apply(self.weights, self.adam_m, self.adam_v, self.fit_steps, self.learning_rate, acc,
                                            1.0 / (chunks * int(count)), self.clip_norm or 0.0, want_norm=self._robust())
        if self._robust():
            self.grad_norms.append(norm)
        return l1, l2

    def _robust(self):
        return self.huber_delta is not None or self.clip_norm is not None

    def _targets(self, n, rows_p, prev_p, next_p, y_act, y_ptr):
        """y_act / y_ptr of the gathered window.  q_sa / p_sp (the current values at the chosen action / pointer) are not
        asked for: the fit's own training-mode forward produces them, so the targets need the forward on next_state only.
        They bootstrap from the target network when there is one; with double_dqn the online blob selects what it
        evaluates; with soft_targets the soft values (and munchausen's log-policy) take the maxima's place."""
        w = self.target.ptr if self.target is not None else self.weights.ptr
        nstep = self.n_step > 1
        ret_p, disc_p = (self._buf["ret"].ptr, self._buf["disc"].ptr) if nstep else (None, None)
        if self.soft_targets is not None:
            alpha, clip = self.munchausen if self.munchausen is not None else (0.0, 0.0)
            self.batch.dqn_targets_soft_into(w, n, rows_p, prev_p, next_p, self.gamma, y_act.ptr, y_ptr.ptr,
                                             self.soft_targets[0], self.soft_targets[1], alpha, clip, ret_p, disc_p)
        elif self.double_dqn:
            self.batch.dqn_targets_double_into(self.weights.ptr, w, n, rows_p, prev_p, next_p, self.gamma, y_act.ptr,
                                               y_ptr.ptr, ret_p, disc_p)
        else:
            self.batch.dqn_targets_into(w, n, rows_p, prev_p, next_p, self.gamma, y_act.ptr, y_ptr.ptr, ret_p, disc_p)

    def _move_target(self):
        """After a fit step: the hard copy of every target_sync-th step or the soft update of each one (on the stream)."""
        if self.target is None:
            return
        if self.target_tau is not None:
            self.batch.policy_blend_weights(self.target, self.weights, self.target_tau)
        elif self.fit_steps % self.target_sync == 0:
            self.batch.policy_blend_weights(self.target, self.weights, 1.0)

    def beta(self):
        """The IS exponent of the next fit step: per_beta -> 1.0 linearly over per_beta_steps fit steps."""
        f = min(1.0, self.fit_steps / float(self.per_beta_steps)) if self.per_beta_steps > 0 else 1.0
        return self.per_beta + (1.0 - self.per_beta) * f
