"""Seeded evolution strategies on the scratch MLP: a population that is never stored (include/ofx.h, "evolution
strategies").

Not in the reference.  Salimans et al. 2017 (OpenAI-ES) with mirrored sampling: one centre genome theta lives in HBM,
member m = 2 i + b of the population is theta +- sigma * eps(i, .) with eps a pure function of (seed, pair, element,
generation) on the project's counter RNG, and a generation ends in a rank-weighted gradient step on theta.  The forward
regenerates the noise of the rows it gathers inside the kernel, so a population of any P costs one genome of memory.

    pair_weights  fitness sums -> the weight of every mirrored pair (centred average ranks): pure numpy, no randomness
    pair_utilities  the same ranks -> (d, s): the pair's weight for the centre and for sigma (adaptive mode)
    ES            owns the ofx_es_* calls of one ArenaBatch; opt-in momentum / Adam and weight decay for the centre,
                  opt-in per-element adaptive sigma
    ESRollout     the generational loop around ShardedRollout's lock-step

eps has variance 1/3 (an Irwin-Hall sum of four uniforms in (-2, 2)): sigma and lr are in units of that eps.  Whether
the fitness rises is an observation (tools/es_time.py records it), not a property any test holds the code to.

Adaptive mode (ES(..., sigma_init=...)) is parameter-exploring policy gradients with symmetric sampling (Sehnke et al.
2010; the separable case of NES): every element e has its own exploration width sigma[e] in HBM beside the centre, member
m = 2 i + b is theta[e] +- sigma[e] * eps(i, e), and ONE kernel steps both from the same noise - the centre on
sum_i d_i eps, sigma on sum_i s_i (eps^2 - 1/3) with s_i = u_{2i} + u_{2i+1}, the pair's utility against the baseline 0
of the centred ranks.  In this mode `lr` multiplies sigma[e] * sum_i d_i eps(i, e) / n_c, which is PEPG's form (the step
of an element is proportional to its own width); the scalar path's estimate is sum_i d_i eps(i, e) / (n_c sigma), OpenAI-ES's
(inversely proportional to the one width).  At equal sigma the two differ by the factor sigma^2: an `lr` tuned for one
mode is not the other's.  sigma[e] itself moves by sigma *= 1 + sigma_lr / n_c * sum_i s_i (eps^2 - 1/3), clamped to
[sigma_min, sigma_max].
"""
import math

import numpy as np

from .evolution import genome_sizes, join_genome, sidecar_path, split_genome
from .rollout import ShardedRollout


def check_members(P, sigma=None):
    """P = 2 n_pairs >= 2 members and, when given, a finite sigma > 0: the library's refusals, checked before it is
    called.  ValueError otherwise; returns int(P)."""
    if int(P) != P or int(P) < 2 or int(P) % 2:
        raise ValueError("P must be even and >= 2 (two members per pair), got %r" % (P,))
    if sigma is not None and not (math.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be finite and > 0, got %r" % (sigma,))
    return int(P)


def check_member_assignment(member_of, N, M, P):
    """member_of as an int32 [N][M] with every value in [-1, P] (-1: the ship is not evolved, P: the centre);
    ValueError otherwise."""
    a = np.asarray(member_of)
    if a.shape != (int(N), int(M)) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("member_of is an integer array [%d][%d], got %s %s" % (N, M, a.dtype, a.shape))
    bad = np.argwhere((a < -1) | (a > P))
    if bad.size:
        i, j = bad[0]
        raise ValueError("member_of[%d][%d] = %d is outside [-1, %d]" % (i, j, a[i, j], P))
    return np.ascontiguousarray(a, dtype=np.int32)


def _ranked_pairs(sum, count):
    """(complete bool [P/2], u, n_c) behind pair_weights and pair_utilities: the centred average ranks u float64
    [n_c/2][2] of the complete pairs' members, None when there is nothing to rank (n_c < 2 or all means equal)."""
    s, c = np.asarray(sum, np.int64), np.asarray(count, np.int64)
    if s.ndim != 1 or s.shape != c.shape or s.shape[0] < 2:
        raise ValueError("sum and count are [P] or [P + 1] arrays, got %s and %s" % (s.shape, c.shape))
    n_pairs = s.shape[0] // 2
    s, c = s[:2 * n_pairs].reshape(n_pairs, 2), c[:2 * n_pairs].reshape(n_pairs, 2)
    complete = (c > 0).all(axis=1)
    n_c = 2 * int(complete.sum())
    if n_c < 2:
        return complete, None, n_c
    mean = (s[complete] / c[complete]).ravel()
    values, inverse, counts = np.unique(mean, return_inverse=True, return_counts=True)
    if values.size == 1:
        return complete, None, n_c
    below = np.cumsum(counts) - counts                     # members ranked strictly below each distinct mean
    rank = (below + (counts - 1) / 2.0)[inverse]           # the average of the ranks a tied group covers
    return complete, (rank / (n_c - 1) - 0.5).reshape(-1, 2), n_c


def pair_weights(sum, count):
    """The weight d_i of every mirrored pair from the device's fitness sums: (d float64 [P/2], n_c).

    sum, count: [P] or [P + 1] (slot P, the centre, is ignored).  A pair is COMPLETE when both its members were flown
    (count > 0); n_c is the number of members of complete pairs.  Those members are ranked by mean fitness sum / count,
    ascending from 0, with AVERAGE ranks for ties (scores are small integers: ties are the common case), then
        u_m = r_m / (n_c - 1) - 0.5        d_i = u_{2i} - u_{2i+1}
    so a tied pair weighs exactly 0, the weights lie in [-1, 1] and swapping a pair's fitness negates its weight.
    Incomplete pairs get 0; n_c < 2 or all means equal gives all zeros.  Pure numpy, no randomness."""
    complete, u, n_c = _ranked_pairs(sum, count)
    d = np.zeros(complete.shape[0], np.float64)
    if u is not None:
        d[complete] = u[:, 0] - u[:, 1]
    return d, n_c


def pair_utilities(sum, count):
    """(d float64 [P/2], s float64 [P/2], n_c) for the adaptive step: d and n_c exactly pair_weights', and
        s_i = u_{2i} + u_{2i+1}
    for complete pairs - the pair's mean utility against the baseline, which is 0 because the ranks are centred (the u
    of the n_c members sum to 0).  A pair both of whose members beat the median has s > 0 and widens sigma where its
    noise was large; swapping a pair's fitness leaves s and negates d.  Incomplete pairs get 0; n_c < 2 or all means
    equal gives all zeros.  Pure numpy, no randomness."""
    complete, u, n_c = _ranked_pairs(sum, count)
    d, w = np.zeros(complete.shape[0], np.float64), np.zeros(complete.shape[0], np.float64)
    if u is not None:
        d[complete] = u[:, 0] - u[:, 1]
        w[complete] = u[:, 0] + u[:, 1]
    return d, w, n_c


def es_meta(layers, seed):
    return {"layers": [int(v) for v in layers], "seed": int(seed)}


def check_es_meta(meta, shape, dtype, layers, seed, path="the checkpoint"):
    """ES.load's refusals, before the centre is touched: ValueError naming the first field of the sidecar `meta` (or of
    the array: its shape, its dtype) that differs from this ES's - evolution.check_population_meta without P."""
    want = es_meta(layers, seed)
    for field in ("layers", "seed"):
        if field not in meta:
            raise ValueError("%s: the sidecar has no field %r" % (path, field))
        got = [int(v) for v in meta[field]] if field == "layers" else int(meta[field])
        if got != want[field]:
            raise ValueError("%s: %s is %r, this ES's is %r" % (path, field, got, want[field]))
    elements = sum(genome_sizes(layers))
    if tuple(shape) != (elements,):
        raise ValueError("%s: shape is %r, a centre of %d elements is %r" % (path, tuple(shape), elements, (elements,)))
    if np.dtype(dtype) != np.float64:
        raise ValueError("%s: dtype is %s, a centre is float64" % (path, np.dtype(dtype)))


OPTIMIZERS = ("momentum", "adam")


def check_optimizer(optimizer, beta1, beta2, adam_eps, weight_decay, adaptive=False):
    """ES's optimiser arguments, checked before the library is touched: ValueError naming the argument.  `adaptive`: the
    step is ofx_es_sigma_step's, whose PLAIN rule has a decay term."""
    if optimizer is not None and optimizer not in OPTIMIZERS:
        raise ValueError("optimizer must be None, 'momentum' or 'adam', got %r" % (optimizer,))
    for name, beta in (("beta1", beta1), ("beta2", beta2)):
        if not (math.isfinite(beta) and 0.0 <= beta < 1.0):
            raise ValueError("%s must be in [0, 1), got %r" % (name, beta))
    if not (math.isfinite(adam_eps) and adam_eps > 0):
        raise ValueError("adam_eps must be finite and > 0, got %r" % (adam_eps,))
    if not (math.isfinite(weight_decay) and weight_decay >= 0):
        raise ValueError("weight_decay must be finite and >= 0, got %r" % (weight_decay,))
    if weight_decay != 0 and optimizer is None and not adaptive:
        raise ValueError("weight_decay needs an optimizer: the bare update has no decay term")


def step_scalars(optimizer, lr, sigma, n_c, t, beta1, beta2):
    """(gscale, alpha, c1, k1, c2, k2) of ofx_es_step at step t (1-based), in Python floats and in this order; Adam's
    bias correction is folded into the step size."""
    return (1.0 / (int(n_c) * float(sigma)),) + step_law(optimizer, lr, t, beta1, beta2)[1:]


def step_law(optimizer, lr, t, beta1, beta2):
    """(rule, alpha, c1, k1, c2, k2): the library's rule constant of `optimizer` and the scalars of its law at step t
    (1-based), in Python floats.  None is the PLAIN rule of ofx_es_sigma_step: the step is lr times the estimate."""
    from . import _native as nat
    if optimizer is None:
        return nat.ES_RULE_PLAIN, float(lr), 0.0, 1.0, 0.0, 1.0
    k1, k2 = 1.0 - beta1, 1.0 - beta2
    if optimizer == "momentum":
        return nat.ES_RULE_MOMENTUM, float(lr), float(beta1), k1, float(beta2), k2
    alpha = float(lr) * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    return nat.ES_RULE_ADAM, alpha, float(beta1), k1, float(beta2), k2


def es_opt_meta(optimizer, beta1, beta2, adam_eps, weight_decay, steps):
    return {"rule": optimizer, "beta1": float(beta1), "beta2": float(beta2), "eps": float(adam_eps),
            "weight_decay": float(weight_decay), "steps": int(steps)}


def check_es_opt_meta(meta, want, shape=None, dtype=None, elements=None, path="the checkpoint"):
    """ES.load's refusals about the optimiser, before anything is touched: ValueError naming the first field that
    differs.  `meta` is the sidecar, `want` this ES's es_opt_meta (None: no optimiser).  The block must be there exactly
    when this ES has an optimiser, and equal `want` in everything but `steps`; shape / dtype, when given, are those of
    the moments' array, float64 [2][elements].  Returns the checkpoint's step count (0 without an optimiser)."""
    block = _check_block(meta, "optimizer", want, ("rule", "beta1", "beta2", "eps", "weight_decay"),
                         "an optimizer block, this ES has no optimizer",
                         want and "this ES's optimizer is %r" % (want["rule"],), path)
    if block is None:
        return 0
    steps = block.get("steps")
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 0:
        raise ValueError("%s: the optimizer block's steps must be an integer >= 0, got %r" % (path, steps))
    _check_array(shape, dtype, (2, elements), "the moments'", "m and v of %d elements are" % (elements or 0),
                 "they are", path)
    return steps


def _check_block(meta, name, want, fields, unwanted, missing, path):
    """The sidecar's block `name` against this ES's `want` (None: no such state): there exactly when wanted, and equal
    in every one of `fields` (a string as it is, a number as a float).  Returns the block, None when none is wanted."""
    block = meta.get(name)
    if want is None:
        if block is not None:
            raise ValueError("%s: the sidecar has %s" % (path, unwanted))
        return None
    if block is None:
        raise ValueError("%s: the sidecar has no %s block, %s" % (path, name, missing))
    for field in fields:
        if field not in block:
            raise ValueError("%s: the %s block has no field %r" % (path, name, field))
        got = block[field] if isinstance(want[field], str) else float(block[field])
        if got != want[field]:
            raise ValueError("%s: %s %s is %r, this ES's is %r" % (path, name, field, got, want[field]))
    return block


def _check_array(shape, dtype, want_shape, whose, of, it_is, path):
    """shape / dtype, when given, of the array a block comes with: float64 `want_shape`."""
    if shape is not None and tuple(shape) != want_shape:
        raise ValueError("%s: %s shape is %r, %s %r" % (path, whose, tuple(shape), of, want_shape))
    if dtype is not None and np.dtype(dtype) != np.float64:
        raise ValueError("%s: %s dtype is %s, %s float64" % (path, whose, np.dtype(dtype), it_is))


def moments_path(path):
    return path + ".opt.npy"


def check_sigma_args(sigma_init, sigma_lr, sigma_min, sigma_max):
    """ES's adaptive-sigma arguments, checked before the library is touched: ValueError naming the argument.  Returns
    None when sigma_init is None (no adaptation), else (sigma_init, sigma_lr, sigma_min, sigma_max) as floats with the
    defaults sigma_min = sigma_init / 64 and sigma_max = sigma_init * 4 filled in."""
    if sigma_init is None:
        if sigma_min is not None or sigma_max is not None:
            raise ValueError("sigma_min and sigma_max need sigma_init: without it sigma is not adapted")
        return None
    if not (math.isfinite(sigma_init) and sigma_init > 0):
        raise ValueError("sigma_init must be finite and > 0, got %r" % (sigma_init,))
    if not (math.isfinite(sigma_lr) and sigma_lr >= 0):
        raise ValueError("sigma_lr must be finite and >= 0, got %r" % (sigma_lr,))
    lo = float(sigma_init) / 64 if sigma_min is None else sigma_min
    hi = float(sigma_init) * 4 if sigma_max is None else sigma_max
    if not (math.isfinite(lo) and lo > 0):
        raise ValueError("sigma_min must be finite and > 0, got %r" % (sigma_min,))
    if not (math.isfinite(hi) and hi >= lo):
        raise ValueError("sigma_max must be finite and >= sigma_min, got %r (sigma_min %r)" % (sigma_max, lo))
    if not (lo <= sigma_init <= hi):
        raise ValueError("sigma_init must lie in [sigma_min, sigma_max] = [%r, %r], got %r" % (lo, hi, sigma_init))
    return float(sigma_init), float(sigma_lr), float(lo), float(hi)


def es_sigma_meta(sigma_lr, sigma_min, sigma_max):
    return {"lr": float(sigma_lr), "min": float(sigma_min), "max": float(sigma_max)}


def check_es_sigma_meta(meta, want, shape=None, dtype=None, elements=None, path="the checkpoint"):
    """ES.load's refusals about the sigma vector, before anything is touched: ValueError naming the first field that
    differs.  `meta` is the sidecar, `want` this ES's es_sigma_meta (None: not adaptive).  The "sigma" block must be
    there exactly when this ES is adaptive, and equal `want`; shape / dtype, when given, are those of the sigma array,
    float64 [elements]."""
    if _check_block(meta, "sigma", want, ("lr", "min", "max"), "a sigma block, this ES does not adapt sigma",
                    "this ES adapts sigma", path) is not None:
        _check_array(shape, dtype, (elements,), "the sigma array's", "a sigma of %d elements is" % (elements or 0),
                     "it is", path)


def sigma_path(path):
    return path + ".sigma.npy"


def check_sigma_mode(adaptive, sigma, es="the ES", how="", how_not=""):
    """sigma is the caller's number, or None exactly when the ES adapts its own: nothing is silently ignored."""
    if adaptive and sigma is not None:
        raise ValueError("sigma must be None: %s adapts sigma per element%s, got %r" % (es, how, sigma))
    if not adaptive and sigma is None:
        raise ValueError("sigma must be a number: %s does not adapt sigma%s" % (es, how_not))


class ES:
    """One ES centre of the scratch MLP `layers` on the device of `batch` (an ArenaBatch), beside any Population the
    batch holds; initialised to the fresh genome of slot 0 from `seed` (the law of Population's init).

    Every member's noise is keyed by (seed, pair, element, generation): a run is reproducible, and no member is stored.

    optimizer  None (default): `update` is the bare step theta += lr / (n_c sigma) * sum_i d_i eps(i, .), call for call
               what it always was.  "momentum" or "adam": the centre gets the moments m and v in HBM (3 genomes instead
               of 1, still at any P) and `update` feeds the estimate minus weight_decay * theta through ofx_es_step
               (include/ofx.h states the law); `opt_steps` counts the steps, 1-based, and is the t of Adam's bias
               correction.  beta1 is the momentum (both rules), beta2 and adam_eps are Adam's.
    sigma_init  None (default): one scalar sigma, the caller's, at every call.  A number turns ADAPTATION on
               (`adaptive`): the centre gets a width per element in HBM (one more genome), every element sigma_init, and
               act / member / update take sigma=None and go to the ofx_es_sigma_* calls; `update` needs the pair
               utilities `s` beside `d` (pair_utilities) and steps theta and sigma in one kernel (include/ofx.h states
               the law; the module docstring what `lr` multiplies here).  sigma_lr is the rate of the sigma step,
               sigma_min / sigma_max its clamp (defaults sigma_init / 64 and sigma_init * 4).  Works with optimizer=None
               (the PLAIN rule, which then also takes weight_decay), "momentum" and "adam"."""

    def __init__(self, batch, layers, seed, optimizer=None, beta1=0.9, beta2=0.999, adam_eps=1e-8, weight_decay=0.0,
                 init=True, sigma_init=None, sigma_lr=0.2, sigma_min=None, sigma_max=None):
        from .engine import DeviceBuffer
        adapt = check_sigma_args(sigma_init, sigma_lr, sigma_min, sigma_max)
        check_optimizer(optimizer, beta1, beta2, adam_eps, weight_decay, adaptive=adapt is not None)
        self.b = batch
        self.layers = [int(v) for v in layers]
        self.seed = int(seed)
        self.n_weights, self.n_biases = genome_sizes(self.layers)
        self.optimizer = optimizer
        self.beta1, self.beta2, self.adam_eps = float(beta1), float(beta2), float(adam_eps)
        self.weight_decay = float(weight_decay)
        self.opt_steps = 0
        batch.es_create(self.layers)
        self.adaptive = adapt is not None
        if optimizer is not None:
            batch.es_opt_create()
        if self.adaptive:
            self.sigma_init, self.sigma_lr, self.sigma_min, self.sigma_max = adapt
            batch.es_sigma_create(self.sigma_init)
        self.n_stats = 5 if self.adaptive else 3 if optimizer is not None else 0   # the sums a step leaves (step_stats)
        if self.n_stats:
            self._stats = DeviceBuffer(self.n_stats * 8).upload(np.zeros(self.n_stats, np.float64))
        self._member_of = DeviceBuffer(batch.N * batch.M * 4)
        self.P, self.member_of = None, None
        self._sum = self._count = None
        self._queue = self._queue_mask = None     # the member queue's (next, completed) and its ships (queue_begin)
        self.queue_total = None
        if init:
            self.init()

    def close(self):
        if self.b is not None:
            self.b.es_destroy()
            self.b = None

    # ---------------------------------------------------------------- the centre and its members
    def init(self, generation=0):
        self.b.es_init(self.seed, generation)

    def centre(self):
        """(weights_layers, biases_layers) of the centre: lists of numpy arrays in the reference's shapes."""
        return split_genome(self.layers, *self.b.es_get(self.n_weights, self.n_biases))

    def set_centre(self, weights_layers, biases_layers):
        self.b.es_set(*join_genome(self.layers, weights_layers, biases_layers))

    def moments(self):
        """(m, v) of the optimiser, each (weights_layers, biases_layers) in the shapes of centre().  Synchronises."""
        self._has_optimizer()
        m, v = self.b.es_opt_get(self.n_weights, self.n_biases)
        return split_genome(self.layers, *m), split_genome(self.layers, *v)

    def set_moments(self, m, v):
        """Put back what moments() returned."""
        self._has_optimizer()
        self.b.es_opt_set(*(join_genome(self.layers, *m) + join_genome(self.layers, *v)))

    def _has_optimizer(self):
        if self.optimizer is None:
            raise ValueError("this ES has no optimizer: construct it with optimizer='momentum' or 'adam'")

    def sigmas(self):
        """(weights_layers, biases_layers) of the sigma vector, in the shapes of centre().  Synchronises."""
        self._is_adaptive()
        return split_genome(self.layers, *self.b.es_sigma_get(self.n_weights, self.n_biases))

    def set_sigmas(self, weights_layers, biases_layers):
        """Put back what sigmas() returned; every element finite and > 0."""
        self._is_adaptive()
        self.b.es_sigma_set(*join_genome(self.layers, weights_layers, biases_layers))

    def _is_adaptive(self):
        if not self.adaptive:
            raise ValueError("this ES does not adapt sigma: construct it with sigma_init")

    def _check_sigma(self, sigma):
        check_sigma_mode(self.adaptive, sigma, "this ES", " (sigma_init)", " (no sigma_init)")

    def member(self, m, P, sigma, generation):
        """(weights_layers, biases_layers) of member m of P at `generation` (m == P: the centre), materialised on the
        device: what Population.set_genome takes.  Adaptive: sigma is None."""
        self._check_sigma(sigma)
        P = check_members(P, sigma)
        if not (0 <= int(m) <= P):
            raise ValueError("member %d outside [0, %d]" % (m, P))
        if self.adaptive:
            return split_genome(self.layers, *self.b.es_sigma_member(m, P, self.seed, generation, self.n_weights,
                                                                     self.n_biases))
        return split_genome(self.layers, *self.b.es_member(m, P, sigma, self.seed, generation, self.n_weights,
                                                           self.n_biases))

    # ------------------------------------------------------------ the device calls
    def assign(self, member_of, P):
        """Which member flies which ship: numpy int [N][M], values in [-1, P] (P: the centre), checked before the upload.
        The fitness buffers are sized for P + 1 slots; a new P starts them at zero."""
        from .engine import DeviceBuffer
        P = check_members(P)
        a = check_member_assignment(member_of, self.b.N, self.b.M, P)
        self.b.sync()
        if P != self.P:
            self._sum = DeviceBuffer(8 * (P + 1)).upload(np.zeros(P + 1, np.int64))
            self._count = DeviceBuffer(4 * (P + 1)).upload(np.zeros(P + 1, np.int32))
            self.P = P
        self._member_of.upload(a)
        self.member_of = a

    def _assigned(self):
        if self.P is None:
            raise ValueError("no assignment yet: call assign(member_of, P) first")

    def act(self, sigma, generation, y_ptr=None):
        """Overwrite the evolved ships' entries of the batch's action array (after bot_actions, before step).  Adaptive:
        sigma is None."""
        self._check_sigma(sigma)
        self._assigned()
        check_members(self.P, sigma)
        if self.adaptive:
            self.b.es_sigma_act(self._member_of.ptr, self.P, self.seed, generation, y_ptr=y_ptr)
            return
        self.b.es_act(self._member_of.ptr, self.P, sigma, self.seed, generation, y_ptr=y_ptr)

    def fitness(self, reset=False):
        """After a restart: add what every assigned ship banked to its member's sum and count (slot P: the centre)."""
        self._assigned()
        self.b.es_fitness(self._member_of.ptr, self.P, self._sum, self._count, reset)

    def fitness_host(self):
        """(sum int64 [P + 1], count int32 [P + 1]) - what a generation brings to the host.  Synchronises."""
        self._assigned()
        self.b.sync()
        return self._sum.download(np.int64, (self.P + 1,)), self._count.download(np.int32, (self.P + 1,))

    def load_fitness(self, sum, count):
        """Put back what fitness_host returned (a resumed run)."""
        self._assigned()
        s, c = np.asarray(sum, np.int64), np.asarray(count, np.int32)
        if s.shape != (self.P + 1,) or c.shape != (self.P + 1,):
            raise ValueError("sum and count are [%d] arrays, got %s and %s" % (self.P + 1, s.shape, c.shape))
        self.b.sync()
        self._sum.upload(s)
        self._count.upload(c)

    # ------------------------------------------------------------ the member queue (ofx_es_requeue)
    def queue_begin(self, queue_mask, P, total):
        """Start a queue of `total` tickets over the assignment made by assign(member_of, P): ticket t is member t % P,
        so total = E * P flies every member E times.  queue_mask: numpy [N][M], nonzero where a ship draws from the
        queue; it is uploaded, member_of becomes -1 on those ships (the other entries of the caller's assignment stay),
        and sum, count and the queue's (next, completed) start at zero.  Synchronises."""
        from .engine import DeviceBuffer
        self._assigned()
        if check_members(P) != self.P:
            raise ValueError("P is %d, the assignment was made for %d: call assign first" % (P, self.P))
        if int(total) != total or int(total) < 0:
            raise ValueError("total must be an integer >= 0, got %r" % (total,))
        q = np.asarray(queue_mask)
        if q.shape != (self.b.N, self.b.M):
            raise ValueError("queue_mask is an array [%d][%d], got %s" % (self.b.N, self.b.M, q.shape))
        q = np.ascontiguousarray(q != 0, dtype=np.uint8)
        a = self.member_of.copy()
        a[q != 0] = -1
        self.b.sync()
        if self._queue is None:
            self._queue_mask, self._queue = DeviceBuffer(q.nbytes), DeviceBuffer(16)
        self._queue_mask.upload(q)
        self._member_of.upload(a)
        self._sum.upload(np.zeros(self.P + 1, np.int64))
        self._count.upload(np.zeros(self.P + 1, np.int32))
        self._queue.upload(np.zeros(2, np.int64))
        self.queue_total = int(total)

    def _queued(self):
        if self._queue is None:
            raise ValueError("no queue yet: call queue_begin(queue_mask, P, total) first")

    def requeue(self, bank=True):
        """After restart_finished / restart_arenas: the ships of the restarted arenas bank what they scored to the member
        they flew (bank) and the queue's ships take the next tickets, -1 when none is left.  Does not synchronise."""
        self._queued()
        self.b.es_requeue(self._member_of.ptr, self._queue_mask.ptr, self.P, self.queue_total, self._queue, self._sum,
                          self._count, bank)

    def queue_host(self):
        """(next, completed): the tickets handed out and the member evaluations banked so far.  Synchronises."""
        self._queued()
        self.b.sync()
        nxt, completed = self._queue.download(np.int64, (2,))
        return int(nxt), int(completed)

    def member_of_host(self):
        """member_of as the device holds it now (requeue rewrites it), int32 [N][M].  Synchronises."""
        self._assigned()
        self.b.sync()
        return self._member_of.download(np.int32, (self.b.N, self.b.M))

    def load_queue(self, member_of, queue):
        """Put back what member_of_host and queue_host returned (a resumed run), after queue_begin.  The queue must
        satisfy 0 <= completed <= next <= total.  The host copy `member_of` stays the assignment assign() was given:
        under the queue only the device holds who flies what (member_of_host)."""
        self._queued()
        a = check_member_assignment(member_of, self.b.N, self.b.M, self.P)
        q = np.asarray([int(v) for v in queue], np.int64)
        if q.shape != (2,) or not (0 <= q[1] <= q[0] <= self.queue_total):
            raise ValueError("queue is (next, completed) with 0 <= completed <= next <= total = %d, got %r"
                             % (self.queue_total, queue))
        self.b.sync()
        self._member_of.upload(a)
        self._queue.upload(q)

    def update(self, d, lr, sigma, n_c, generation, s=None):
        """The generation step theta += lr / (n_c sigma) * sum_i d_i eps(i, .) on the noise of `generation`, the one the
        members flew with; (d, n_c) from pair_weights.  The scale is computed in Python floats, in that order.

        With an optimizer: opt_steps += 1 and the step goes through ofx_es_step with the scalars of step_scalars; its
        three sums wait in the ES's stats buffer for step_stats().

        Adaptive: sigma is None and `s` (pair_utilities) is required; theta and sigma[e] step in one kernel
        (ofx_es_sigma_step) with gscale = 1.0 / n_c - sigma[e] is inside the law - srate = sigma_lr / n_c, alpha as
        step_scalars computes it (lr itself for the PLAIN rule); opt_steps counts as before (with an optimizer) and
        the five sums wait for step_stats()."""
        self._check_sigma(sigma)
        if self.adaptive and s is None:
            raise ValueError("s is required: the adaptive step needs the pair utilities (pair_utilities)")
        if not self.adaptive and s is not None:
            raise ValueError("s must be None: this ES does not adapt sigma (no sigma_init)")
        d = np.asarray(d, np.float64)
        if d.ndim != 1 or d.shape[0] < 1 or not np.isfinite(d).all():
            raise ValueError("d is a finite float64 [P / 2], got %s" % (d.shape,))
        check_members(2 * d.shape[0], sigma)
        if int(n_c) < 2 or not math.isfinite(lr):
            raise ValueError("update needs n_c >= 2 and a finite lr, got n_c = %r, lr = %r" % (n_c, lr))
        if self.adaptive:
            s = np.asarray(s, np.float64)
            if s.shape != d.shape or not np.isfinite(s).all():
                raise ValueError("s is a finite float64 [P / 2] like d, got %s" % (s.shape,))
        elif self.optimizer is None:
            scale = float(lr) / (int(n_c) * float(sigma))
            self.b.es_update(d, scale, self.seed, generation)
            return
        if self.optimizer is not None:
            self.opt_steps += 1
        rule, alpha, c1, k1, c2, k2 = step_law(self.optimizer, lr, self.opt_steps, self.beta1, self.beta2)
        if self.adaptive:
            self.b.es_sigma_step(d, s, rule, 1.0 / int(n_c), self.weight_decay, alpha, c1, k1, c2, k2, self.adam_eps,
                                 self.sigma_lr / int(n_c), self.sigma_min, self.sigma_max, self.seed, generation,
                                 stats_ptr=self._stats.ptr)
        else:
            self.b.es_step(d, rule, 1.0 / (int(n_c) * float(sigma)), self.weight_decay, alpha, c1, k1, c2, k2,
                           self.adam_eps, self.seed, generation, stats_ptr=self._stats.ptr)

    def step_stats(self):
        """(grad_sq, step_sq, centre_sq) of the last optimiser step: the sums over the genome of q^2 (the estimate minus
        the decay term), of step^2 and of theta'^2, zeros before the first step.  Adaptive: five numbers - those three, the
        sum of sigma'^2 and the number of elements a clamp changed.  Synchronises."""
        if not self.adaptive:
            self._has_optimizer()
        self.b.sync()
        return tuple(float(x) for x in self._stats.download(np.float64, (self.n_stats,)))

    # ------------------------------------------------------------ checkpoint of the centre
    def save(self, path):
        """The centre as ONE .npy at `path`, float64 [n_weights + n_biases] in the element order, and the sidecar
        `path + ".json"` with layers and seed.  With an optimizer also `path + ".opt.npy"`, float64 [2][elements], m
        then v in the element order, and the sidecar's "optimizer" block (rule, betas, eps, weight_decay, steps).
        Adaptive: also `path + ".sigma.npy"`, float64 [elements] in the element order, and the sidecar's "sigma" block
        (lr, min, max).  Returns path."""
        import json
        w, b = self.b.es_get(self.n_weights, self.n_biases)
        meta = es_meta(self.layers, self.seed)
        for block, want, file_of, _, get, _ in self._vectors():
            if want is not None:
                a = get()
                with open(file_of(path), "wb") as f:
                    np.save(f, a)
                meta[block] = want
        with open(path, "wb") as f:
            np.save(f, np.concatenate([w, b]))
        with open(sidecar_path(path), "w") as f:
            json.dump(meta, f)
        return path

    def _opt_meta(self):
        return None if self.optimizer is None else es_opt_meta(self.optimizer, self.beta1, self.beta2, self.adam_eps,
                                                               self.weight_decay, self.opt_steps)

    def _sigma_meta(self):
        return es_sigma_meta(self.sigma_lr, self.sigma_min, self.sigma_max) if self.adaptive else None

    def _vectors(self):
        """What a checkpoint may hold beside the centre, in the order save and load take it: (the sidecar's block, this
        ES's meta for it or None, the array's file, the checker, the array from the device, the array to the device)."""
        b, nw, nb = self.b, self.n_weights, self.n_biases
        return (("optimizer", self._opt_meta(), moments_path, check_es_opt_meta,
                 lambda: np.stack([np.concatenate(x) for x in b.es_opt_get(nw, nb)]),
                 lambda a: b.es_opt_set(a[0, :nw], a[0, nw:], a[1, :nw], a[1, nw:])),
                ("sigma", self._sigma_meta(), sigma_path, check_es_sigma_meta,
                 lambda: np.concatenate(b.es_sigma_get(nw, nb)),
                 lambda a: b.es_sigma_set(a[:nw], a[nw:])))

    def load(self, path):
        """The centre `save` wrote, into this ES.  ValueError naming the field, with the centre untouched, when the
        checkpoint's layers or seed (or the array's shape or dtype) differ from this ES's - or when its optimizer block
        is missing, unwanted or differs in anything but `steps` (check_es_opt_meta).  With an optimizer the moments and
        opt_steps come back too: the next update is the one the saved run would have made.  The same for the "sigma"
        block and the sigma array (check_es_sigma_meta): every refusal comes before anything is written."""
        import json
        with open(sidecar_path(path)) as f:
            meta = json.load(f)
        arr = np.load(path)
        check_es_meta(meta, arr.shape, arr.dtype, self.layers, self.seed, path)
        vectors = self._vectors()
        # the sidecar first: no array's file is opened for a refusal the sidecar alone decides
        steps = [check(meta, want, path=path) for _, want, _, check, _, _ in vectors][0]
        arrays = []
        for block, want, file_of, check, _, put in vectors:
            if want is not None:
                a = np.load(file_of(path))
                check(meta, want, a.shape, a.dtype, arr.shape[0], path)
                if block == "sigma" and not (np.isfinite(a).all() and (a > 0).all()):
                    raise ValueError("%s: the sigma array holds a value that is not finite and > 0" % path)
                arrays.append((put, a))
        self.b.es_set(arr[:self.n_weights], arr[self.n_weights:])
        for put, a in arrays:
            put(a)
        if self.optimizer is not None:
            self.opt_steps = steps


class ESRollout(ShardedRollout):
    """The generational loop of the evolution strategy: every ship of `ships` in every arena is flown by a member of the
    population of `P` around the centre of `es`, the others by `behaviours`; at each episode end the restart banks the
    scores and the fitness call adds them per member; every `episodes_per_generation` episodes, in this order: the
    2 x (P + 1) fitness numbers come to the host, (best, mean) is appended to `fitness_log`, pair_weights turns them into
    (d, n_c) - kept in `weight_log` - the centre takes its step on the noise of the generation that just flew,
    generation += 1 and the ships are reassigned.  A generation with fewer than two flown members of complete pairs has
    nothing to learn from and leaves the centre as it is.

    member_of[a][ships[k]] = ((arena_base + a) * len(ships) + k + generation) % P, as EvolutionRollout assigns genomes;
    the last `eval_arenas` arenas fly the centre (member P) instead, and their mean banked score per generation goes to
    `centre_log`.  Runs with observe=False; its policy hook is es.act.  Single GPU: with `dist` set it refuses.

    es  an ES on `engine` (or anything with its assign, act, fitness, fitness_host, update; for state_dict also
        load_fitness; for log_steps also step_stats)
    log_steps  opt-in, for an ES with an optimizer: after each generation's update, es.step_stats() - the sums of
        squares of the estimate, the step and the centre - is appended to `step_log` (one download of three doubles per
        stepped generation).
    sigma  a number, or None exactly when es.adaptive: the members then fly with the ES's own sigma per element, the
        generation end uses pair_utilities, `weight_log` keeps (d, s, n_c), es.update gets s=s and, with log_steps,
        `step_log` holds five-tuples (ES.step_stats).
    auto_reset  opt-in (a bool; False: lockstep() makes exactly the calls it always made).  True gives every arena its
        own episodes and takes the members from a queue on the device (include/ofx.h, "the member queue"), so P may
        exceed N * len(ships) and no lock-step is spent on a finished evaluation except in a generation's tail.
        episodes_per_generation is then E, the evaluations per member, and a generation is total = E * P tickets, ticket
        t = member t % P.  The queue mask is `ships` in the first N - eval_arenas arenas, the restart mask `ships` in
        every arena; the evaluation arenas hold member P throughout and bank to slot P on their own restarts.
        A generation BEGINS - at construction after the spawn, and after every update - with es.queue_begin,
        engine.restart_arenas(seed) on all arenas and es.requeue(bank=False): a centre episode cut by the forced restart
        is discarded, centre_log[g] holds only episodes flown wholly by centre g.  Every lockstep() STARTS with
        engine.restart_finished(seed, restart mask, max_ticks=episode_ticks) and es.requeue(bank=True); when tick > 0 and
        tick % poll_every == 0 the two queue counters come to the host (the one synchronisation), and
        completed == total ends the generation: fitness to the host, fitness_log (centre_log), pair_utilities, update,
        step_log, weight_log, generation += 1, then the next generation begins; then the lock-step goes on as ever.  A
        ship whose tickets ran out (member -1) flies its `behaviours` entry until the generation ends.  The global
        episode end never runs: score_log stays empty and engine.episode 0.  `generation_log` holds per generation
        (lock-steps it took, member evaluations banked, centre episodes banked).
    poll_every  an integer >= 1: how often, in lock-steps, auto_reset looks at the queue.
    """

    def __init__(self, engine, es, behaviours, seed, P, sigma, lr, ships=(0,), episodes_per_generation=1, eval_arenas=0,
                 log_steps=False, auto_reset=False, poll_every=8, **kw):
        if not isinstance(auto_reset, (bool, np.bool_)):   # every argument is checked before the first device call
            raise ValueError("auto_reset must be a bool, got %r" % (auto_reset,))
        if isinstance(poll_every, bool) or not isinstance(poll_every, (int, np.integer)) or poll_every < 1:
            raise ValueError("poll_every must be an integer >= 1, got %r" % (poll_every,))
        self.auto_reset, self.poll_every = bool(auto_reset), int(poll_every)
        if kw.get("dist") is not None:
            raise ValueError("ESRollout runs on one GPU: `dist` must be None")
        if kw.get("policy") is not None or kw.get("observe"):
            raise ValueError("ESRollout sets `policy` and runs with observe=False")
        self.ships = [int(i) for i in ships]
        if not self.ships or len(set(self.ships)) != len(self.ships) or not all(0 <= i < engine.M for i in self.ships):
            raise ValueError("ships must be distinct ship slots in [0, %d), got %r" % (engine.M, list(ships)))
        self.adaptive = bool(getattr(es, "adaptive", False))
        check_sigma_mode(self.adaptive, sigma)
        self.P = check_members(P, sigma)
        if not math.isfinite(lr):
            raise ValueError("lr must be finite, got %r" % (lr,))
        if int(episodes_per_generation) < 1:
            raise ValueError("episodes_per_generation must be >= 1, got %r" % (episodes_per_generation,))
        if int(eval_arenas) != eval_arenas or not (0 <= int(eval_arenas) < engine.N):
            raise ValueError("eval_arenas must be in [0, %d): an arena must be left to learn from, got %r"
                             % (engine.N, eval_arenas))
        kw["observe"] = False
        super().__init__(engine, behaviours, seed, **kw)
        self.es = es
        self.sigma, self.lr = (None if sigma is None else float(sigma)), float(lr)
        self.episodes_per_generation, self.eval_arenas = int(episodes_per_generation), int(eval_arenas)
        self.generation = 0
        self.episodes = 0                 # finished episodes of the current generation
        self.fitness_log = []             # (best mean fitness of a member, mean fitness per evolved ship) per generation
        self.centre_log = []              # mean banked score of a centre-flown ship per generation (eval_arenas > 0)
        self.weight_log = []              # (d, n_c) each generation stepped on; adaptive: (d, s, n_c)
        self.log_steps = bool(log_steps)
        self.step_log = []                # (grad_sq, step_sq, centre_sq) per stepped generation (log_steps)
        self.policy = self._fly
        self.generation_log = []          # auto_reset: (lock-steps, member evaluations banked, centre episodes banked)
        if not self.auto_reset:
            self._assign()
            return
        from .engine import DeviceBuffer
        self.total = self.episodes_per_generation * self.P    # tickets of a generation: every member flown E times
        restart = np.zeros((engine.N, engine.M), np.uint8)
        restart[:, self.ships] = 1
        self.queue_mask = restart.copy()
        self.queue_mask[engine.N - self.eval_arenas:] = 0     # the evaluation arenas hold member P throughout
        held = np.full((engine.N, engine.M), -1, np.int32)
        held[restart != self.queue_mask] = self.P
        engine.sync()
        self._restart_mask = DeviceBuffer(restart.nbytes).upload(restart)
        self.es.assign(held, self.P)
        self._generation_begin()

    def _fly(self, engine):
        self.es.act(self.sigma, self.generation)

    # ------------------------------------------------------------ auto_reset: per-arena episodes, members from a queue
    def _generation_begin(self):
        """Every arena starts an episode of its own on fresh tickets; a centre episode cut here is discarded."""
        self.es.queue_begin(self.queue_mask, self.P, self.total)
        self.e.restart_arenas(self.seed)
        self.es.requeue(bank=False)
        self._generation_tick = self.tick

    def lockstep(self):
        if not self.auto_reset:
            return super().lockstep()
        self.e.restart_finished(self.seed, self._restart_mask.ptr, max_ticks=self.episode_ticks)
        self.es.requeue(bank=True)
        if self.tick > 0 and self.tick % self.poll_every == 0:
            if self.es.queue_host()[1] == self.total:
                self._generation_end()
        self._fly_and_step()

    def _generation_end(self):
        s, c = self._learn()
        self.generation_log.append((self.tick - self._generation_tick, int(c[:self.P].sum()), int(c[self.P])))
        self._generation_begin()

    def assignment(self, generation):
        """member_of (int32 [N][M]) of `generation` by the formula; the last eval_arenas arenas fly the centre."""
        e, K = self.e, len(self.ships)
        g = np.full((e.N, e.M), -1, np.int32)
        arena = np.arange(e.arena_base, e.arena_base + e.N, dtype=np.int64)
        for k, ship in enumerate(self.ships):
            g[:, ship] = (arena * K + k + generation) % self.P
            if self.eval_arenas:
                g[e.N - self.eval_arenas:, ship] = self.P
        return g

    def _assign(self):
        self.es.assign(self.assignment(self.generation), self.P)

    def _episode_end(self):
        total = super()._episode_end()
        self.es.fitness(reset=self.episodes == 0)
        self.episodes += 1
        if self.episodes == self.episodes_per_generation:
            self._learn()
            self.episodes = 0
            self._assign()
        return total

    def _learn(self):
        """The end of a generation up to generation += 1: the fitness comes to the host, the logs, the centre's step.
        Returns the (sum, count) it learned from."""
        s, c = self.es.fitness_host()
        ms, mc = s[:self.P], c[:self.P]
        flown = mc > 0
        mean = ms[flown] / mc[flown]
        self.fitness_log.append((float(mean.max()) if flown.any() else float("nan"),
                                 float(ms.sum()) / float(max(int(mc.sum()), 1))))
        if self.eval_arenas:
            self.centre_log.append(float(s[self.P]) / float(c[self.P]) if c[self.P] else float("nan"))
        d, w, n_c = pair_utilities(s, c)                   # d and n_c are pair_weights'
        if n_c >= 2:
            # self.sigma is None exactly when adaptive; a scalar ES, or a stand-in for one, takes no s=
            self.es.update(d, self.lr, self.sigma, n_c, self.generation, **({"s": w} if self.adaptive else {}))
            if self.log_steps:
                self.step_log.append(tuple(self.es.step_stats()))
        self.weight_log.append((d, w, n_c) if self.adaptive else (d, n_c))
        self.generation += 1
        return s, c

    # ------------------------------------------------------------ stop and go on
    def state_dict(self):
        """What a run stopped between two lock-steps needs, beside the centre (ES.save: with an optimizer also its
        moments and step count), to go on bit for bit in fresh handles: the generation and episode counters, the logs
        (step_log only with log_steps), the fitness sums and counts of the running generation, the tick and
        ArenaBatch.state_dict().  Under auto_reset it also carries auto_reset and poll_every (load_state_dict refuses a
        rollout whose own differ, by field, before anything is touched; a state without them was written with the
        option off), member_of as the queue left it, the queue's (next, completed), the arenas' episode counters and
        dead_once marks, generation_log and the tick the running generation began at."""
        s, c = self.es.fitness_host()
        d = {"generation": self.generation, "episodes": self.episodes, "tick": self.tick,
             "fitness_log": list(self.fitness_log), "centre_log": list(self.centre_log),
             "weight_log": [tuple(np.array(x) for x in w[:-1]) + (int(w[-1]),) for w in self.weight_log],
             "score_log": [np.array(t) for t in self.score_log], "fitness_sum": s, "fitness_count": c,
             "engine": self.e.state_dict()}
        if self.log_steps:
            d["step_log"] = list(self.step_log)
        if self.auto_reset:
            # what the queue has handed out, and every arena's own episode (the engine's counters, not in its state_dict)
            auto = self.e.autoreset_state()
            d.update(auto_reset=True, poll_every=self.poll_every, member_of=self.es.member_of_host(), queue=self.es.queue_host(),
                     arena_episode=auto["arena_episode"], dead_once=auto["dead_once"],
                     generation_log=list(self.generation_log), generation_tick=self._generation_tick)
        return d

    def load_state_dict(self, d):
        """Continue the run state_dict() described, on a freshly constructed ESRollout with the same arguments whose ES
        already holds the centre (ES.load)."""
        missing = [k for k in ("generation", "episodes", "tick", "fitness_log", "centre_log", "weight_log", "score_log",
                               "fitness_sum", "fitness_count", "engine") if k not in d]
        if missing:
            raise ValueError("ESRollout.load_state_dict: field %r is missing" % missing[0])
        # a state written with the option off has neither field (poll_every means nothing there)
        for field, mine in (("auto_reset", self.auto_reset), ("poll_every", self.poll_every)):
            saved = d.get(field, False if field == "auto_reset" else mine)
            if saved != mine and (field == "auto_reset" or self.auto_reset):
                raise ValueError("ESRollout.load_state_dict: %s is %r, this rollout's is %r" % (field, saved, mine))
        if self.auto_reset:
            missing = [k for k in ("member_of", "queue", "arena_episode", "dead_once", "generation_log",
                                   "generation_tick") if k not in d]
            if missing:
                raise ValueError("ESRollout.load_state_dict: field %r is missing" % missing[0])
        self.e.load_state_dict(d["engine"])
        self.generation, self.episodes, self.tick = int(d["generation"]), int(d["episodes"]), int(d["tick"])
        self.fitness_log, self.centre_log = list(d["fitness_log"]), list(d["centre_log"])
        self.weight_log = [tuple(np.array(x) for x in w[:-1]) + (int(w[-1]),) for w in d["weight_log"]]
        self.score_log = [np.array(t) for t in d["score_log"]]
        if "step_log" in d:
            self.step_log = [tuple(t) for t in d["step_log"]]
        if self.auto_reset:
            # the construction began a generation of its own: the saved one's tickets and counters replace it
            self.e.load_autoreset_state({"arena_episode": d["arena_episode"], "dead_once": d["dead_once"]})
            self.es.load_queue(d["member_of"], d["queue"])
            self.generation_log = [tuple(int(v) for v in t) for t in d["generation_log"]]
            self._generation_tick = int(d["generation_tick"])
        else:
            self._assign()
        self.es.load_fitness(d["fitness_sum"], d["fitness_count"])
