"""Host stand-ins that run DeviceTrainer.replay() without a GPU and record what it issues (tests/test_replay_calls.py,
tests/record_replay_calls.py): a DeviceBuffer that is an address range and an ArenaBatch that logs every call and returns
canned values.

One log entry is `name(arg, ...)`: every argument of the call after binding it to the real ArenaBatch method's signature
(defaults filled in), scalars as they are, pointers - a buffer object or a raw address - as `buffer name+byte offset`,
resolved against the trainer's scratch (`_buf`) and its weights / adam_m / adam_v / target blobs.  The plain targets are
logged under the C entry's name and arguments (ofx_dqn_targets, ofx_dqn_targets_nstep, without the handle), whether they
arrive through ArenaBatch.dqn_targets_into or, on a tree whose trainer still calls the library itself, through
`native_shim`.

Two things are host housekeeping and not part of the issue order, so they are not log entries: dqn_acc_floats() (a size
query) and the sync() + free() of a scratch buffer that grows (free() checks that the sync came first and takes it out
again).  What grew is pinned instead through the scratch sizes after every replay."""
import inspect
import itertools

import numpy as np

BASE, STRIDE = 1 << 40, 1 << 24          # every buffer owns [ptr, ptr + STRIDE); no scalar argument comes near BASE
N_FLOATS = 8


class HostBuffer:
    count = 0
    log = None                           # the running case's log (free() edits it)

    def __init__(self, nbytes):
        HostBuffer.count += 1
        self.nbytes, self.ptr = int(nbytes), BASE + HostBuffer.count * STRIDE
        self.data = np.zeros(self.nbytes, np.uint8)

    def upload(self, arr):
        b = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        self.data[:b.size] = b
        return self

    def download(self, dtype, shape, offset=0):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self.data[offset:offset + n].view(dtype).reshape(shape).copy()

    def free(self):
        assert HostBuffer.log and HostBuffer.log[-1] == "sync()", "a scratch buffer was freed without a sync before it"
        HostBuffer.log.pop()


def _engine():
    from ofighters_amd.engine import ArenaBatch
    return ArenaBatch


LOGGED = ("sync replay_create replay_prioritize replay_actor_priorities replay_count replay_sample "
          "replay_sample_prioritized replay_gather_valid_into replay_gather_nstep_into replay_window_weights_into "
          "replay_update_priorities replay_sample_global replay_gather_list_into replay_update_priorities_list "
          "dqn_targets_double_into policy_blend_weights dqn_fit dqn_fit_weighted dqn_fit_robust dqn_fit_reference dqn_grad "
          "dqn_apply").split()


class RecordingBatch:
    N, M, W, H = 3, 2, 16, 16
    handle = "handle"

    def __init__(self):
        self.TRANSITION_DTYPE = _engine().TRANSITION_DTYPE
        self.log, self.trainer, self.fits, self.step = [], None, 0, None
        HostBuffer.log = self.log

    # ---- logging
    def _name(self, v):
        p = v if isinstance(v, (int, np.integer)) else v.ptr
        tr = self.trainer
        for name, buf in list(tr._buf.items()) + [(k, getattr(tr, k)) for k in ("weights", "adam_m", "adam_v", "target")]:
            if buf is not None and buf.ptr <= p < buf.ptr + STRIDE:
                return "%s+%d" % (name, p - buf.ptr)
        raise AssertionError("a pointer into no buffer of the trainer: %r" % (v,))

    def _arg(self, v):
        if hasattr(v, "ptr") or (isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and v >= BASE):
            return self._name(v)
        return repr(v.item() if isinstance(v, np.generic) else v)

    def _log(self, name, args):
        self.log.append("%s(%s)" % (name, ", ".join(self._arg(a) for a in args)))

    def __getattr__(self, name):
        if name not in LOGGED:
            raise AttributeError(name)
        sig = inspect.signature(getattr(_engine(), name))

        def call(*args, **kw):
            bound = sig.bind(self, *args, **kw)
            bound.apply_defaults()
            a = dict(bound.arguments)
            a.pop("self")
            self._log(name, a.values())
            return getattr(self, "_r_" + name, lambda a: None)(a)
        return call

    def dqn_targets_into(self, w, n, rows_p, prev_p, next_p, gamma, y_act_p, y_ptr_p, ret_p=None, disc_p=None):
        if ret_p is None:
            self._log("ofx_dqn_targets", (w, n, rows_p, prev_p, next_p, float(gamma), None, None, y_act_p, y_ptr_p))
        else:
            self._log("ofx_dqn_targets_nstep", (w, n, rows_p, prev_p, next_p, ret_p, disc_p, None, None, y_act_p, y_ptr_p))

    def native_shim(self):
        """Stand-ins for `_native.lib` and `_native.check` that log the two target entries like dqn_targets_into."""
        batch = self

        class Lib:
            def __getattr__(self, name):
                assert name in ("ofx_dqn_targets", "ofx_dqn_targets_nstep"), name
                return lambda h, *args: batch._log(name, args)
        return (lambda: Lib()), (lambda rc: None)

    def dqn_acc_floats(self):
        return N_FLOATS + 256

    # ---- canned results
    def _r_replay_create(self, a):
        self.replay_capacity, self.replay_frames = a["capacity"], a["frames"] or a["capacity"] + a["capacity"] // 4 + 2

    def _r_replay_count(self, a):
        return np.array(self.step["cnt"], np.int32), np.zeros(self.N, np.int64)

    def _r_replay_sample(self, a):
        a["n"].upload(np.array(self.step["n_s"], np.int32))
        return a["slot"], a["n"]

    def _r_replay_sample_prioritized(self, a):
        return self._r_replay_sample(a) + (a["is_weight"],)

    def _r_replay_sample_global(self, a):
        return a["arena"], a["slot"], a["is_weight"], self.step["drawn"], self.step["drawn"] + 100

    def _r_replay_gather_valid_into(self, a):
        return a["max_rows"]

    _r_replay_gather_nstep_into = _r_replay_gather_valid_into

    def _loss(self, norm):
        self.fits += 1
        return (self.fits + 0.5, self.fits + 0.25) + ((self.fits + 0.125 if norm else None,) if norm is not None else ())

    def _r_dqn_fit(self, a):
        return self._loss(None)

    _r_dqn_fit_weighted = _r_dqn_fit_reference = _r_dqn_fit

    def _r_dqn_fit_robust(self, a):
        return self._loss(bool(a["huber_delta"]) or bool(a["clip_norm"]))

    def _r_dqn_apply(self, a):
        return self._loss(bool(a["clip_norm"]) if a["want_norm"] is None else bool(a["want_norm"]))


# ------------------------------------------------------------------------------------------------------------ the cases
COMMON = dict(learning_rate=1e-3, batch_size=4, memory_size=16, frames=0, seed=5, fit_batch=8, per_beta_steps=4)
OPTIONS = {"prioritized": dict(prioritized=True), "n_step": dict(n_step=3), "double": dict(double_dqn=True, target_sync=2),
           "huber": dict(huber_delta=1.0), "global": dict(global_sampling=True), "accumulate": dict(accumulate=2),
           "hook": dict(hook="none")}
WINDOW = [dict(cnt=[2, 1, 2], n_s=[2, 1, 2]), dict(cnt=[4, 5, 3], n_s=[4, 3, 3]), dict(cnt=[6, 6, 6], n_s=[4, 4, 4])]
LIST = {1: [dict(drawn=5), dict(drawn=8), dict(drawn=8)], 2: [dict(drawn=5), dict(drawn=16), dict(drawn=13)]}


def _pairwise():
    """A greedy covering of every pair of option values that a trainer accepts (accumulate needs global sampling)."""
    names = list(OPTIONS)
    combos = [c for c in itertools.product((False, True), repeat=len(names))
              if c[names.index("global")] or not c[names.index("accumulate")]]
    pairs = lambda c: {(i, c[i], j, c[j]) for i in range(len(c)) for j in range(i + 1, len(c))}
    left = set().union(*(pairs(c) for c in combos))
    out = []
    while left:
        best = max(combos, key=lambda c: len(pairs(c) & left))       # the first of equals: product order
        left -= pairs(best)
        out.append([n for n, on in zip(names, best) if on])
    return out


def cases():
    """[(name, trainer kwargs, hook, [what the batch returns in each replay], batch_size argument)]"""
    out = []
    for on in _pairwise():
        kw = {}
        for n in on:
            kw.update(OPTIONS[n])
        hook = kw.pop("hook", None)
        sched = LIST[kw.get("accumulate", 1)] if "global" in on else WINDOW
        out.append(("pair:" + ("+".join(on) or "default"), kw, hook, sched, None))
    per = dict(prioritized=True)
    out += [
        ("clip_norm", dict(clip_norm=10.0), None, WINDOW, None),
        ("target_tau", dict(target_tau=0.25), None, WINDOW, None),
        ("reference_quirks", dict(reference_quirks=True), None, WINDOW, None),
        ("reference_quirks:hook_is_not_called", dict(reference_quirks=True), "none", WINDOW, None),
        ("list_fused:prioritized+clip_norm", dict(per, global_sampling=True, clip_norm=10.0), None, LIST[1], None),
        ("list_fused:prioritized", dict(per, global_sampling=True), None, LIST[1], None),
        ("actor_priorities", dict(per, actor_priorities=True), None, WINDOW, None),
        ("hook_returns_2:window", dict(per, clip_norm=10.0), 2, WINDOW, None),
        ("hook_returns_2:list", dict(per, global_sampling=True, accumulate=2, huber_delta=1.0), 2, LIST[2], None),
        ("batch_size_argument", {}, None, [dict(cnt=[2, 2, 2], n_s=[2, 2, 1]), dict(cnt=[9, 9, 9], n_s=[2, 2, 2]),
                                           dict(cnt=[9, 9, 9], n_s=[2, 2, 2])], 2),
        ("window_sizes", dict(per, n_step=3), None,
         [dict(cnt=[0, 0, 0]), dict(cnt=[1, 0, 1], n_s=[0, 0, 0])] + WINDOW + [dict(cnt=[9, 9, 9], n_s=[4, 4, 3])], None),
        ("list_sizes", dict(per, n_step=3, global_sampling=True, accumulate=2, target_sync=2), None,
         [dict(drawn=0), dict(drawn=5), dict(drawn=21), dict(drawn=16)], None),
        ("list_sizes:uniform_three_chunks", dict(global_sampling=True, accumulate=3), None,
         [dict(drawn=21), dict(drawn=24), dict(drawn=5)], None),
    ]
    return out


def run_case(tr_module, setattr_, kw, hook, sched, batch_size):
    """Build a DeviceTrainer of `tr_module` on the stand-ins (setattr_(object, name, value) patches, e.g.
    monkeypatch.setattr) and replay once per schedule entry -> {"setup": log, "replays": [{log, returned, state}]}."""
    setattr_(tr_module, "DeviceBuffer", HostBuffer)
    batch = RecordingBatch()
    if not hasattr(_engine(), "dqn_targets_into"):              # a trainer that calls the library itself for the targets
        from ofighters_amd import _native
        lib, check = batch.native_shim()
        setattr_(_native, "lib", lib), setattr_(_native, "check", check)
    tr = tr_module.DeviceTrainer(batch, np.arange(N_FLOATS, dtype=np.float32), **dict(COMMON, **kw))
    batch.trainer = tr
    if hook is not None:
        def grad_hook(trainer, acc):
            batch._log("grad_hook", (acc,))
            return None if hook == "none" else hook
        tr.grad_hook = grad_hook
    out = {"setup": list(batch.log), "replays": []}
    for step in sched:
        del batch.log[:]
        batch.step = step
        returned = tr.replay() if batch_size is None else tr.replay(batch_size)
        out["replays"].append({"log": list(batch.log), "returned": returned,
                               "state": {"fit_steps": tr.fit_steps, "draws": tr.draws, "losses": list(tr.losses),
                                         "grad_norms": list(tr.grad_norms),
                                         "scratch": {k: b.nbytes for k, b in sorted(tr._buf.items())}}})
    return out
