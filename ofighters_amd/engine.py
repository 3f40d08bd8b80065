"""ArenaBatch - host-side driver of N lock-stepped arenas on one MI355X.

The batched analogue of ``Battleground`` (lib/battleground.py:10-173): the
per-tick order is the reference's ``frame()`` (battleground.py:163-166)

    request_actions -> generate_frame(actions) -> Observation(battleground)

with the GUI's laser clean-up between ticks (lib/ofighters.py:619-625,702-707)
and ``restart()`` between episodes.  All arithmetic happens in libofx.so
(hand-written HIP); this module only marshals numpy / device pointers.
"""
import ctypes as C

import numpy as np

from . import _native as nat

_FIELD_DTYPE = {
    nat.F_SHIP_X: np.int32, nat.F_SHIP_Y: np.int32, nat.F_SHIP_PX: np.int32, nat.F_SHIP_PY: np.int32,
    nat.F_SHIP_ALIVE: np.uint8, nat.F_REWARD: np.int32, nat.F_SCORE: np.int32, nat.F_N_LASERS: np.int32,
    nat.F_LASER_X: np.float64, nat.F_LASER_Y: np.float64, nat.F_LASER_OWNER: np.uint8,
    nat.F_LASER_DEAD: np.uint8, nat.F_KILLER: np.int16, nat.F_TIME: np.int32, nat.F_LAST_SCORES: np.int32,
    nat.F_HULL: np.int32, nat.F_LASER_DX: np.float64, nat.F_LASER_DY: np.float64, nat.F_OBS_REWARD: np.int32,
}
_MAP_DTYPE = {nat.MAP_U8: np.uint8, nat.MAP_F32: np.float32, nat.MAP_F64: np.float64, nat.MAP_BITS: np.uint8}

ACTION_DTYPE = np.dtype([("px", np.int32), ("py", np.int32), ("shoot", np.uint8), ("thrust", np.uint8),
                         ("valid", np.uint8), ("_pad", np.uint8)])
assert ACTION_DTYPE.itemsize == C.sizeof(nat.OfxAction) == 12


class DeviceBuffer:
    """A raw HBM allocation owned by the host side (ofx_malloc / ofx_free)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        nat.check(nat.lib().ofx_malloc(C.byref(p), self.nbytes))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes > self.nbytes:
            raise Exception("DeviceBuffer.upload: %d bytes into a %d byte buffer" % (arr.nbytes, self.nbytes))
        nat.check(nat.lib().ofx_memcpy_h2d(self.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return self

    def download(self, dtype, shape, offset=0):
        """Copy `shape` elements of `dtype` starting `offset` bytes into the buffer back to the host."""
        out = np.empty(shape, dtype=dtype)
        if offset < 0 or offset + out.nbytes > self.nbytes:
            raise Exception("DeviceBuffer.download: %d bytes at offset %d from a %d byte buffer" % (out.nbytes, offset, self.nbytes))
        nat.check(nat.lib().ofx_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.ptr + int(offset), out.nbytes))
        return out

    def free(self):
        if getattr(self, "ptr", None):
            nat.lib().ofx_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _ArrayInterface:
    """__cuda_array_interface__ (version 3) over a raw HBM pointer; `owner` keeps the memory's owner alive."""

    def __init__(self, ptr, shape, typestr, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 3,
                                         "strides": None}


def pack_actions(valid, shoot, thrust, px, py):
    """numpy -> [N][M] ofx_action records (lib/action.py:12-56; valid=0 is None)."""
    valid = np.asarray(valid)
    a = np.zeros(valid.shape, dtype=ACTION_DTYPE)
    a["valid"] = valid
    a["shoot"] = shoot
    a["thrust"] = thrust
    a["px"] = px
    a["py"] = py
    return a


def _f64_out(*sizes):
    """(arrays, pointers): fresh float64 arrays of `sizes` for the library to fill - a genome's (weights, biases)."""
    arrays = [np.empty(int(n), np.float64) for n in sizes]
    return arrays, [a.ctypes.data_as(C.c_void_p) for a in arrays]


def _f64_in(*values):
    """(arrays, pointers): `values` as contiguous float64 for the library to read; the arrays live as long as the
    caller holds them."""
    arrays = [np.ascontiguousarray(v, dtype=np.float64) for v in values]
    return arrays, [a.ctypes.data_as(C.c_void_p) for a in arrays]


def check_pool_pairs(what, packed, pool_pairs):
    """The size argument of the packed frame store (replay_create's pool_pairs, DeviceTrainer's memory_pool_pairs): an
    integer >= 0 and no bool, and 0 unless the packed store is asked for.  ValueError otherwise; returns it as int."""
    if isinstance(pool_pairs, bool) or not isinstance(pool_pairs, (int, np.integer)) or pool_pairs < 0:
        raise ValueError("%s must be an integer >= 0 (0 = the library's default), got %r" % (what, pool_pairs))
    if pool_pairs and not packed:
        raise ValueError("%s = %d sizes the packed frame store, which is off (packed / packed_memory)" % (what, pool_pairs))
    return int(pool_pairs)


# include/ofx.h, "symmetry augmentation": an element g in 0 .. 7 is three bits applied in this order to a position
OFX_SYM_TRANSPOSE, OFX_SYM_FLIP_X, OFX_SYM_FLIP_Y = 1, 2, 4
SYM_INVERSE = (0, 1, 2, 5, 4, 3, 6, 7)
SYM_COMPOSE = ((0, 1, 2, 3, 4, 5, 6, 7), (1, 0, 3, 2, 5, 4, 7, 6), (2, 5, 0, 7, 6, 1, 4, 3), (3, 4, 1, 6, 7, 0, 5, 2),
               (4, 3, 6, 1, 0, 7, 2, 5), (5, 2, 7, 0, 1, 6, 3, 4), (6, 7, 4, 5, 2, 3, 0, 1), (7, 6, 5, 4, 3, 2, 1, 0))
"""SYM_COMPOSE[a][b]: the one element that does a first, then b."""


class ArenaBatch:
    def __init__(self, n_arenas, n_ships=8, **cfg):
        self.cfg = nat.default_config(n_arenas=n_arenas, n_ships=n_ships, **cfg)
        h = C.c_void_p()
        nat.check(nat.lib().ofx_create(C.byref(self.cfg), C.byref(h)))
        self._h = h.value
        self.N, self.M, self.L = self.cfg.n_arenas, self.cfg.n_ships, self.cfg.laser_cap
        self.W, self.H = self.cfg.width, self.cfg.height
        self.arena_base = self.cfg.arena_base
        self._actions = DeviceBuffer(self.N * self.M * ACTION_DTYPE.itemsize)
        self._draws = None
        self._head = None
        self._done = None
        self.tick = 0
        self.episode = 0

    # ---------------------------------------------------------------- lifetime
    def close(self):
        if getattr(self, "_h", None):
            nat.lib().ofx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def sync(self):
        nat.check(nat.lib().ofx_sync(self._h))

    # --------------------------------------------------------- spawn / restart
    def _draw_buf(self, draws):
        d = np.ascontiguousarray(draws, dtype=np.int32).reshape(self.N, self.M, 2)
        if self._draws is None:
            self._draws = DeviceBuffer(d.nbytes)
        self.sync()  # raw copies are not ordered with the handle's stream
        return self._draws.upload(d).ptr

    def spawn(self, draws):
        """Battleground.__init__ positions: draws [N,M,2] = randint(0,W), randint(0,H)."""
        nat.check(nat.lib().ofx_spawn(self._h, self._draw_buf(draws)))
        self.tick = 0

    def spawn_random(self, seed):
        nat.check(nat.lib().ofx_spawn_random(self._h, seed))
        self.tick = 0

    def restart(self, draws, arena_mask=None):
        mptr = None
        if arena_mask is not None:
            m = np.ascontiguousarray(arena_mask, dtype=np.uint8).reshape(self.N)
            self.sync()
            self._mask = DeviceBuffer(m.nbytes).upload(m)
            mptr = self._mask.ptr
        nat.check(nat.lib().ofx_restart(self._h, self._draw_buf(draws), mptr))
        self.episode += 1

    def restart_random(self, seed):
        self.episode += 1
        nat.check(nat.lib().ofx_restart_random(self._h, seed, self.episode))

    # ------------------------------------------- per-arena episodes (include/ofx.h: the contract)
    def restart_finished(self, seed, ship_mask_ptr=None, max_ticks=0, seen_buf=None, group_buf=None, n_groups=1,
                         sums_buf=None):
        """Restart, on the device, the arenas whose own episode is over (ofx_restart_finished): every ship selected by
        the device uint8 [N][M] at ship_mask_ptr (None = all) was seen destroyed by an earlier call already, or the
        arena's clock F_TIME has reached max_ticks (0 = no clock).  Call it once per decision, before bot_actions and
        the forward.  seen_buf (DeviceBuffer, uint8 [N][M], agents_first_done's latches) is cleared for the restarted
        arenas; sums_buf (DeviceBuffer, int64 [n_groups][M+2], zeroed by the caller) accumulates per group of group_buf
        (DeviceBuffer, int32 [N]; None = one group) the banked scores, the episodes and their lock-steps.  `episode` is
        not advanced: every arena counts its own (autoreset_state).  Does not synchronise."""
        nat.check(nat.lib().ofx_restart_finished(self._h, seed, ship_mask_ptr, int(max_ticks),
                                                 seen_buf.ptr if seen_buf is not None else None,
                                                 group_buf.ptr if group_buf is not None else None, int(n_groups),
                                                 sums_buf.ptr if sums_buf is not None else None))

    def restart_arenas(self, seed, mask_buf=None):
        """Restart, on the device, the arenas the caller names (ofx_restart_arenas): mask_buf is a DeviceBuffer of uint8
        [N], None = every arena.  restart_finished's restart without its decision, its sums and its `seen`; `restarted`
        of autoreset_state() becomes the mask.  `episode` is not advanced.  Does not synchronise."""
        nat.check(nat.lib().ofx_restart_arenas(self._h, seed, mask_buf.ptr if mask_buf is not None else None))

    def autoreset_state(self):
        """restart_finished's state on the host: arena_episode uint32 [N], dead_once uint8 [N][M] and restarted uint8
        [N], the arenas the last call restarted.  OfxError (OFX_ERR_STATE) before the first call.  Synchronises."""
        ep, dead, res = np.empty(self.N, np.uint32), np.empty((self.N, self.M), np.uint8), np.empty(self.N, np.uint8)
        nat.check(nat.lib().ofx_autoreset_state_host(self._h, *[a.ctypes.data_as(C.c_void_p) for a in (ep, dead, res)]))
        return {"arena_episode": ep, "dead_once": dead, "restarted": res}

    def load_autoreset_state(self, d):
        """Upload autoreset_state()'s arena_episode and dead_once (a checkpoint's); shapes and dtypes are checked first."""
        arrs = []
        for name, dt, shape in (("arena_episode", np.uint32, (self.N,)), ("dead_once", np.uint8, (self.N, self.M))):
            if name not in d:
                raise ValueError("ArenaBatch.load_autoreset_state: %r is missing" % name)
            a = np.asarray(d[name])
            if a.dtype != dt or a.shape != shape:
                raise ValueError("ArenaBatch.load_autoreset_state: %r is %s %s, this batch holds %s %s"
                                 % (name, a.dtype, a.shape, np.dtype(dt), shape))
            arrs.append(np.ascontiguousarray(a))
        nat.check(nat.lib().ofx_autoreset_set_state(self._h, *[a.ctypes.data_as(C.c_void_p) for a in arrs]))

    def set_ships(self, x=None, y=None, px=None, py=None):
        """Crafted starts (test / fixture use): overwrite ship fields [N,M]."""
        for f, v in ((nat.F_SHIP_X, x), (nat.F_SHIP_Y, y), (nat.F_SHIP_PX, px), (nat.F_SHIP_PY, py)):
            if v is not None:
                a = np.ascontiguousarray(v, dtype=np.int32).reshape(self.N, self.M)
                self.sync()
                nat.check(nat.lib().ofx_memcpy_h2d(nat.lib().ofx_device_ptr(self._h, f),
                                                   a.ctypes.data_as(C.c_void_p), a.nbytes))

    # -------------------------------------------------------------------- tick
    def step(self, actions=None, actions_ptr=None):
        """One lock-step.  `actions`: structured array [N,M] (pack_actions) or
        `actions_ptr`: device pointer to [N][M] ofx_action."""
        if actions is None and actions_ptr is None:
            actions_ptr = self._actions.ptr  # the device buffer bot_actions / policy_actions wrote
        if actions_ptr is None:
            a = np.ascontiguousarray(actions, dtype=ACTION_DTYPE).reshape(self.N, self.M)
            self.sync()  # the previous tick may still be reading the buffer
            actions_ptr = self._actions.upload(a).ptr
        nat.check(nat.lib().ofx_step(self._h, actions_ptr))
        self.tick += 1

    def bot_actions(self, behaviours, seed, tick=None, out_ptr=None):
        """Scripted bots on device (agents/agent.py:99-155 laws) -> device actions."""
        b = np.array([nat.BEHAVIOURS[x] if not isinstance(x, (int, np.integer)) else int(x) for x in behaviours],
                     dtype=np.int32)
        if b.shape != (self.M,):
            raise Exception("behaviours must have one entry per ship")
        out_ptr = out_ptr or self._actions.ptr
        nat.check(nat.lib().ofx_bot_actions(self._h, b.ctypes.data_as(C.c_void_p), seed,
                                            self.tick if tick is None else tick, out_ptr))
        return out_ptr

    def rollout(self, behaviours, seed, tick0, n_ticks, observe=None):
        """Battleground.run for scripted bots (battleground.py:169-173): n_ticks lock-steps enqueued by ONE host call
        (ofx_rollout); `observe` = a nat.MAP_* type to rasterise after every lock-step, None = step only (all lock-steps
        inside one kernel launch).  Bit-identical to n_ticks x (bot_actions, step[, rasterise])."""
        b = np.array([nat.BEHAVIOURS[x] if not isinstance(x, (int, np.integer)) else int(x) for x in behaviours],
                     dtype=np.int32)
        if b.shape != (self.M,):
            raise Exception("behaviours must have one entry per ship")
        nat.check(nat.lib().ofx_rollout(self._h, b.ctypes.data_as(C.c_void_p), seed, int(tick0), int(n_ticks),
                                        -1 if observe is None else int(observe)))
        self.tick += int(n_ticks)

    def step_repeat(self, behaviours, seed, tick0, n_ticks, hold_mask_ptr=None, actions_ptr=None, span_reward_ptr=None,
                    observe=None):
        """Action repeat (ofx_step_repeat): n_ticks lock-steps in ONE kernel launch.  The ships marked in the device
        uint8 [N][M] at hold_mask_ptr hold their entry of the device action array for the whole span (actions_ptr=None
        with a mask: the batch's own buffer, the one policy_actions wrote), the others follow `behaviours` lock-step by
        lock-step; span_reward_ptr (device int32 [N][M]) receives every ship's rewards summed over the span; `observe`
        = a nat.MAP_* type rasterised once after the last lock-step.  Bit-identical to n_ticks x (bot_actions, the
        held entries overwritten, step).  Advances `tick` by n_ticks; does not synchronise."""
        b = np.array([nat.BEHAVIOURS[x] if not isinstance(x, (int, np.integer)) else int(x) for x in behaviours],
                     dtype=np.int32)
        if b.shape != (self.M,):
            raise Exception("behaviours must have one entry per ship")
        if hold_mask_ptr is not None and actions_ptr is None:
            actions_ptr = self._actions.ptr
        nat.check(nat.lib().ofx_step_repeat(self._h, b.ctypes.data_as(C.c_void_p), seed, int(tick0), int(n_ticks),
                                            hold_mask_ptr, actions_ptr, span_reward_ptr,
                                            -1 if observe is None else int(observe)))
        self.tick += int(n_ticks)

    def actions_host(self):
        self.sync()
        return self._actions.download(ACTION_DTYPE, (self.N, self.M))

    # ------------------------------------------------------------- observation
    def rasterise(self, map_type=nat.MAP_U8, ship_ptr=None, laser_ptr=None):
        nat.check(nat.lib().ofx_rasterise(self._h, map_type, ship_ptr, laser_ptr))

    def maps_host(self, map_type=nat.MAP_U8):
        """(ship_map, laser_map) as numpy [N,W,H] ([N,W*H/8] for MAP_BITS)."""
        self.rasterise(map_type)
        per = nat.lib().ofx_map_bytes(self._h, map_type)
        dt = np.dtype(_MAP_DTYPE[map_type])
        shape = (self.N, per) if map_type == nat.MAP_BITS else (self.N, self.W, self.H)
        out = []
        for which in (0, 1):
            a = np.empty(shape, dtype=dt)
            self.sync()
            nat.check(nat.lib().ofx_memcpy_d2h(a.ctypes.data_as(C.c_void_p),
                                               nat.lib().ofx_map_ptr(self._h, map_type, which), a.nbytes))
            out.append(a)
        return out

    def observe_head(self):
        """obs.vector[:8] for every ship + done flags (observation.py:101-123)."""
        if self._head is None:
            self._head = DeviceBuffer(self.N * self.M * 8 * 8)
            self._done = DeviceBuffer(self.N * self.M)
        nat.check(nat.lib().ofx_observe_head(self._h, self._head.ptr, self._done.ptr))
        self.sync()
        return (self._head.download(np.float64, (self.N, self.M, 8)),
                self._done.download(np.uint8, (self.N, self.M)))

    # ------------------------------------------------------------ state access
    def get(self, field):
        dt = np.dtype(_FIELD_DTYPE[field])
        nbytes = nat.lib().ofx_field_bytes(self._h, field)
        a = np.empty(nbytes // dt.itemsize, dtype=dt)
        nat.check(nat.lib().ofx_get_host(self._h, field, a.ctypes.data_as(C.c_void_p), nbytes))
        return a if field in (nat.F_N_LASERS, nat.F_TIME) else a.reshape(self.N, -1)

    def device_ptr(self, field):
        return nat.lib().ofx_device_ptr(self._h, field)

    # ------------------------------------------------------------ zero-copy views
    # The batched form of the reference's plugin seam ("any object with .play(obs)", agents/agent.py:34-37): an external
    # policy - a torch module, say - reads the maps and the ships' state where they lie in HBM and writes its actions
    # into the [N][M] ofx_action array the next step() reads.  Nothing is copied; see include/ofx.h (ofx_field_desc) for
    # the ownership rule: the CONTENTS are those of the last step / rasterise and the next one overwrites them in place.
    # torch must have been imported BEFORE the library was loaded (both bring a HIP runtime of the same soname and the
    # process keeps the first one: with libofx's first, torch finds no GPU).
    def _view(self, desc, keep=None):
        import torch
        if not torch.cuda.is_available():
            raise Exception("ArenaBatch tensor views need torch's GPU runtime: import torch before ofighters_amd loads "
                            "libofx.so (the process keeps the first HIP runtime it loads)")
        shape = tuple(int(desc.shape[i]) for i in range(desc.ndim))
        holder = _ArrayInterface(desc.data, shape, nat.DT_TYPESTR[desc.dtype], keep or self)
        return torch.as_tensor(holder, device=torch.device("cuda", int(desc.device)))

    def tensor(self, field):
        """State field `field` (nat.F_*) as a torch tensor over the handle's own memory: [N][M], [N][L] or [N]."""
        d = nat.OfxTensorDesc()
        nat.check(nat.lib().ofx_field_desc(self._h, int(field), C.byref(d)))
        return self._view(d)

    def maps_tensor(self, map_type=nat.MAP_U8):
        """(ship_map, laser_map) of the handle's internal buffers of `map_type` as torch tensors [N][W = y][H = x]
        ([N][W * H / 8] uint8 for MAP_BITS), filled by rasterise(map_type)."""
        out = []
        for which in (0, 1):
            d = nat.OfxTensorDesc()
            nat.check(nat.lib().ofx_map_desc(self._h, int(map_type), which, C.byref(d)))
            out.append(self._view(d))
        return tuple(out)

    def actions_tensor(self):
        """The [N][M] ofx_action array step() reads by default, as views of its fields: px, py int32 [N][M]; shoot,
        thrust, valid uint8 [N][M] (lib/action.py:12-56; valid = 0 is the reference's None)."""
        import torch
        d = nat.OfxTensorDesc()
        d.data, d.dtype, d.itemsize, d.ndim, d.device = self._actions.ptr, nat.DT_U8, 1, 3, self.cfg.device
        d.shape[0], d.shape[1], d.shape[2] = self.N, self.M, ACTION_DTYPE.itemsize
        raw = self._view(d, keep=self._actions)
        words = raw.view(torch.int32)                    # [N][M][3]: px, py, (shoot | thrust << 8 | valid << 16)
        return {"px": words[..., 0], "py": words[..., 1], "shoot": raw[..., 8], "thrust": raw[..., 9],
                "valid": raw[..., 10], "raw": raw}

    def torch_stream(self):
        """The handle's HIP stream as a torch stream: `with torch.cuda.stream(batch.torch_stream()):` puts a policy's
        kernels in order with step() / rasterise() (the handle's stream does not synchronise with torch's default one)."""
        import torch
        return torch.cuda.ExternalStream(int(nat.lib().ofx_stream(self._h)), device=torch.device("cuda", self.cfg.device))

    def overflow_count(self):
        v = C.c_int64(0)
        nat.check(nat.lib().ofx_overflow_count(self._h, C.byref(v)))
        return v.value

    def episode_scores_host(self):
        """int64 [M+1]: per-slot sums banked at the last restart + arena count."""
        buf = DeviceBuffer(8 * (self.M + 1))
        nat.check(nat.lib().ofx_episode_scores(self._h, buf.ptr))
        self.sync()
        return buf.download(np.int64, (self.M + 1,))

    episode_scores = episode_scores_host

    def episode_scores_into(self, dev_ptr):
        nat.check(nat.lib().ofx_episode_scores(self._h, dev_ptr))

    def episode_scores_grouped(self, group_buf, n_groups):
        """int64 [n_groups][M+1]: episode_scores per group of arenas.  group_buf: DeviceBuffer, int32 [N], the group of
        every local arena (-1, or any value outside [0, n_groups): not counted); the last column counts the arenas."""
        n_groups = int(n_groups)
        buf = DeviceBuffer(8 * max(1, n_groups) * (self.M + 1))
        nat.check(nat.lib().ofx_episode_scores_grouped(self._h, group_buf.ptr, n_groups, buf.ptr))
        self.sync()
        return buf.download(np.int64, (n_groups, self.M + 1))

    # ------------------------------------------------------------------ timing
    def timer_start(self):
        nat.check(nat.lib().ofx_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float(0)
        nat.check(nat.lib().ofx_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def event_record(self, idx):
        nat.check(nat.lib().ofx_event_record(self._h, idx))

    def event_elapsed(self, a, b):
        ms = C.c_float(0)
        nat.check(nat.lib().ofx_event_elapsed(self._h, a, b, C.byref(ms)))
        return ms.value

    # ------------------------------------------------------------------ policy
    def policy_layout(self):
        d = nat.OfxPolicyDesc()
        nat.check(nat.lib().ofx_policy_layout(self._h, C.byref(d)))
        n = d.n_tensors
        return list(d.offset[:n]), list(d.count[:n]), d.n_floats

    def policy_forward(self, weights_ptr, ship_mask_ptr=None, act_ptr=None, iaction_ptr=None, ipointer_ptr=None,
                       heat_ptr=None):
        """Bi-head forward for every (arena, ship) on the CURRENT state (device pointers;
        None iaction / ipointer are kept by the handle for policy_explore / policy_actions / replay_capture)."""
        nat.check(nat.lib().ofx_policy_forward(self._h, weights_ptr, ship_mask_ptr, act_ptr, iaction_ptr,
                                               ipointer_ptr, heat_ptr))

    def policy_pin_weights(self, weights_ptr):
        """Prepare (fold BatchNorm, build the phase weights) once: every following forward on this blob reuses it.
        None unpins.  (The reference keeps one compiled Keras model between predicts, qlearnIA_V2.py:308.)"""
        nat.check(nat.lib().ofx_policy_pin_weights(self._h, weights_ptr))

    def set_option(self, option, value):
        """Diagnostic switches of the forward: nat.OPT_TRUNK_PLAIN, nat.OPT_FRAMES_REF (reference variants)."""
        nat.check(nat.lib().ofx_set_option(self._h, int(option), int(value)))

    def policy_trunk_stats(self):
        """OPT_TRUNK_SPARSE: (M-tiles run, M-tiles, table passes run, table passes) since the last call."""
        v = (C.c_int64 * 4)()
        nat.check(nat.lib().ofx_policy_trunk_stats(self._h, v))
        return tuple(int(x) for x in v)

    def policy_trunk_stats3(self):
        """OPT_TRUNK_SPARSE = 1: (M-tiles run, M-tiles) of the streaming conv3 since the last call."""
        run, total = C.c_int64(), C.c_int64()
        nat.check(nat.lib().ofx_policy_trunk_stats3(self._h, C.byref(run), C.byref(total)))
        return int(run.value), int(total.value)

    def policy_trunk_features(self):
        """The trunk's output [N][25][25][8] of the forward that has just run on all N arenas (diagnostic: read out of the
        forward's workspace, valid only right behind it)."""
        out = np.empty((self.N, 25, 25, 8), np.float32)
        self.sync()
        nat.check(nat.lib().ofx_policy_trunk_features(self._h, self.N, self.M, out.ctypes.data_as(C.c_void_p)))
        return out

    def policy_actions(self, out_ptr=None, iaction_ptr=None, ipointer_ptr=None, ship_mask_ptr=None):
        """QlearnIA.play packing of the last forward into [N][M] ofx_action."""
        out_ptr = out_ptr or self._actions.ptr
        nat.check(nat.lib().ofx_policy_actions(self._h, iaction_ptr, ipointer_ptr, ship_mask_ptr, out_ptr))
        return out_ptr

    def policy_forward_host(self, weights, ship_mask=None, want_heat=False):
        """Convenience for tests / the facade: numpy in, numpy out."""
        S = self.N * self.M
        w = np.ascontiguousarray(weights, np.float32)
        dw = DeviceBuffer(w.nbytes).upload(w)
        dm = None
        if ship_mask is not None:
            m = np.ascontiguousarray(ship_mask, np.uint8).reshape(S)
            dm = DeviceBuffer(m.nbytes).upload(m)
        da, di, dp = DeviceBuffer(8 * S), DeviceBuffer(4 * S), DeviceBuffer(8 * S)
        dh = DeviceBuffer(4 * S * self.W * self.H) if want_heat else None
        self.sync()
        self.policy_forward(dw.ptr, dm.ptr if dm else None, da.ptr, di.ptr, dp.ptr, dh.ptr if dh else None)
        self.sync()
        out = dict(act=da.download(np.float32, (self.N, self.M, 2)), iaction=di.download(np.int32, (self.N, self.M)),
                   ipointer=dp.download(np.int32, (self.N, self.M, 2)))
        if want_heat:
            out["heat"] = dh.download(np.float32, (self.N, self.M, self.W, self.H))
        return out

    # ------------------------------------------------------------------ facade support
    def step_packed(self, packed):
        """packed int32 [N,M,5] = valid, shoot, thrust, px, py (the facade's Action.packed())."""
        p = np.asarray(packed, np.int32).reshape(self.N, self.M, 5)
        self.step(pack_actions(p[..., 0], p[..., 1], p[..., 2], p[..., 3], p[..., 4]))

    def snapshot(self):
        g = self.get
        return dict(x=g(nat.F_SHIP_X), y=g(nat.F_SHIP_Y), px=g(nat.F_SHIP_PX), py=g(nat.F_SHIP_PY),
                    alive=g(nat.F_SHIP_ALIVE), hull=g(nat.F_HULL), reward=g(nat.F_REWARD), score=g(nat.F_SCORE),
                    n_lasers=g(nat.F_N_LASERS), lx=g(nat.F_LASER_X), ly=g(nat.F_LASER_Y),
                    lowner=g(nat.F_LASER_OWNER), ldead=g(nat.F_LASER_DEAD))

    def maps_f64(self):
        sm, lm = self.maps_host(nat.MAP_U8)
        return sm.astype(np.float64), lm.astype(np.float64)

    def policy_profile(self, event_base):
        nat.check(nat.lib().ofx_policy_profile(self._h, event_base))

    # ------------------------------------------------------------ replay memory
    TRANSITION_DTYPE = np.dtype([("tick_prev", np.int32), ("tick_next", np.int32), ("frame_prev", np.int32),
                                 ("frame_next", np.int32), ("ship", np.int32),
                                 ("iaction", np.int32), ("px", np.int32), ("py", np.int32), ("reward", np.int32),
                                 ("done", np.int32), ("head_prev", np.float32, 8), ("head_next", np.float32, 8)])

    STORE_STATS = ("packed", "pool_pairs", "live_max", "live_sum", "evicted", "store_bytes")

    def replay_create(self, capacity=400, frames=0, packed=False, pool_pairs=0):
        """Trainer.memory = deque(maxlen=memory_size) per arena (qlearnIA_V2.py:58).

        packed=True (opt-in, exact) keeps the stored observation maps as the (word index, word) pairs of their nonzero
        words in a cyclic pool of `pool_pairs` pairs per arena instead of the dense frame ring - a tenth of its HBM at the
        default pool_pairs = 0 (max(512 * frames, 4 * W*H/32)); any other value must be >= 4 * W*H/32 and < 2^31.  Every
        reader returns the same bytes as from the dense ring; when an arena's live frames outgrow its pool the oldest are
        released early and the rows that need them stop being eligible, exactly like rows whose frame was overwritten
        (replay_store_stats()["evicted"] counts them).  include/ofx.h, "packed frame store", has the rule."""
        pool_pairs = check_pool_pairs("replay_create: pool_pairs", packed, pool_pairs)
        if packed:
            nat.check(nat.lib().ofx_replay_create_packed(self._h, int(capacity), int(frames), pool_pairs))
        else:
            nat.check(nat.lib().ofx_replay_create(self._h, int(capacity), int(frames)))
        self.replay_capacity = int(capacity)
        self.replay_frames = int(frames) if frames else int(capacity) + int(capacity) // 4 + 2   # include/ofx.h
        self.replay_prioritized = False

    def replay_store_stats(self):
        """The frame store of the replay memory (ofx_replay_store_stats; synchronises): packed (1 / 0), pool_pairs per
        arena, live_max / live_sum (pairs of the live frames: the fullest arena, all arenas), evicted (frames released
        early since replay_create; per process, not carried by a checkpoint) and store_bytes (HBM held).  A dense memory
        reports 0 for all but store_bytes."""
        v = (C.c_int64 * 6)()
        nat.check(nat.lib().ofx_replay_store_stats(self._h, v))
        return dict(zip(self.STORE_STATS, (int(x) for x in v)))

    def replay_capture(self, tick, ship_mask_ptr=None, iaction_ptr=None, ipointer_ptr=None):
        """QlearnIA.play bookkeeping + Trainer.remember for this lock-step; call before step()."""
        nat.check(nat.lib().ofx_replay_capture(self._h, int(tick), ship_mask_ptr, iaction_ptr, ipointer_ptr))

    def replay_reward_source(self, reward_ptr):
        """Where the captures take a completed row's reward from: a device int32 [N][M] the caller owns (step_repeat's
        span_reward), None = the state's reward field, the default.  Element 0 of the stored observation head stays the
        state's reward either way.  Does not synchronise."""
        nat.check(nat.lib().ofx_replay_reward_source(self._h, reward_ptr))

    def agents_first_done(self, ship_mask_ptr, seen_buf):
        """How many selected ships are destroyed now and not yet marked in `seen_buf` (DeviceBuffer, uint8 [N][M]); marks
        them.  QlearnIA.play's `if obs.done` (qlearnIA_V2.py:376-384) for all learning agents: one int crosses to the host."""
        n = C.c_int32(0)
        nat.check(nat.lib().ofx_agents_first_done(self._h, ship_mask_ptr, seen_buf.ptr, C.byref(n)))
        return n.value

    def replay_count(self):
        cnt = np.empty(self.N, np.int32)
        app = np.empty(self.N, np.int64)
        nat.check(nat.lib().ofx_replay_count(self._h, cnt.ctypes.data_as(C.c_void_p), app.ctypes.data_as(C.c_void_p)))
        return cnt, app

    def replay_rows(self, arena):
        """list(memory) of one arena, oldest first, as a structured array."""
        rows = np.zeros(self.replay_capacity, self.TRANSITION_DTYPE)
        n = C.c_int32()
        nat.check(nat.lib().ofx_replay_rows_host(self._h, int(arena), rows.ctypes.data_as(C.c_void_p), C.byref(n)))
        return rows[:n.value]

    def replay_frame(self, arena, tick):
        """(ship_map, laser_map) uint8 [H][W] of a stored lock-step."""
        nb = self.W * self.H // 8
        a, b = np.empty(nb, np.uint8), np.empty(nb, np.uint8)
        nat.check(nat.lib().ofx_replay_frame_host(self._h, int(arena), int(tick), a.ctypes.data_as(C.c_void_p),
                                                   b.ctypes.data_as(C.c_void_p)))
        un = lambda x: np.unpackbits(x, bitorder="little").reshape(self.H, self.W)
        return un(a), un(b)

    def replay_sample(self, seed, draw, batch, slot=None, n=None):
        """random.sample(memory, min(batch, len)) per arena -> (slot DeviceBuffer [N][batch], n DeviceBuffer [N]); the
        caller may hand in both buffers (DeviceTrainer keeps them between replays)."""
        if slot is None:
            slot = DeviceBuffer(4 * self.N * batch)
        if n is None:
            n = DeviceBuffer(4 * self.N)
        nat.check(nat.lib().ofx_replay_sample(self._h, seed, int(draw), int(batch), slot.ptr, n.ptr))
        return slot, n

    def replay_gather(self, slot, batch, with_maps=True):
        """Materialise sampled rows: (rows [N][batch], bits_prev, bits_next uint32 [N][batch][2][W*H/32]) on the host."""
        rows = DeviceBuffer(self.N * batch * self.TRANSITION_DTYPE.itemsize)
        words = self.W * self.H // 32
        bp = DeviceBuffer(4 * self.N * batch * 2 * words) if with_maps else None
        bn = DeviceBuffer(4 * self.N * batch * 2 * words) if with_maps else None
        nat.check(nat.lib().ofx_replay_gather(self._h, slot.ptr, int(batch), rows.ptr, bp.ptr if bp else None,
                                               bn.ptr if bn else None))
        self.sync()
        out = [rows.download(self.TRANSITION_DTYPE, (self.N, batch))]
        if with_maps:
            out += [bp.download(np.uint32, (self.N, batch, 2, words)), bn.download(np.uint32, (self.N, batch, 2, words))]
        return out

    def replay_gather_device(self, slot, batch):
        """Like replay_gather but the minibatch stays in HBM: (rows, bits_prev, bits_next) DeviceBuffers."""
        rows = DeviceBuffer(self.N * batch * self.TRANSITION_DTYPE.itemsize)
        words = self.W * self.H // 32
        bp, bn = DeviceBuffer(4 * self.N * batch * 2 * words), DeviceBuffer(4 * self.N * batch * 2 * words)
        nat.check(nat.lib().ofx_replay_gather(self._h, slot.ptr, int(batch), rows.ptr, bp.ptr, bn.ptr))
        return rows, bp, bn

    def replay_gather_valid(self, slot, n_sampled, batch, first, max_rows):
        """The sampled minibatch without padding rows, packed in (arena, j) order and kept in HBM: entries first ..
        first + max_rows - 1 -> (rows, bits_prev, bits_next, n_rows).  Trainer.replay never pads (qlearnIA_V2.py:241-243)."""
        rows = DeviceBuffer(max_rows * self.TRANSITION_DTYPE.itemsize)
        words = self.W * self.H // 32
        bp, bn = DeviceBuffer(4 * max_rows * 2 * words), DeviceBuffer(4 * max_rows * 2 * words)
        n = C.c_int32()
        nat.check(nat.lib().ofx_replay_gather_valid(self._h, slot.ptr, n_sampled.ptr, int(batch), int(first), int(max_rows),
                                                     rows.ptr, bp.ptr, bn.ptr, C.byref(n)))
        return rows, bp, bn, n.value

    def replay_gather_valid_into(self, slot, n_sampled, batch, first, max_rows, rows, bits_prev, bits_next):
        """replay_gather_valid into the caller's DeviceBuffers (a trainer keeps them between replays); returns n_rows."""
        n = C.c_int32()
        nat.check(nat.lib().ofx_replay_gather_valid(self._h, slot.ptr, n_sampled.ptr, int(batch), int(first), int(max_rows),
                                                     rows.ptr, bits_prev.ptr, bits_next.ptr, C.byref(n)))
        return n.value

    # ------------------------------------------------------------ prioritized replay (include/ofx.h: the contract)
    def replay_prioritize(self, alpha=0.6, eps=1e-3):
        """Enable prioritized experience replay on the memory: masses p^alpha per row, new rows at the running max."""
        nat.check(nat.lib().ofx_replay_prioritize(self._h, float(alpha), float(eps)))
        self.replay_prioritized = True

    def replay_sample_prioritized(self, seed, draw, batch, beta, slot=None, n=None, is_weight=None):
        """Stratified proportional sample per arena -> (slot [N][batch], n [N], is_weight [N][batch]) DeviceBuffers;
        slot / n as replay_sample, is_weight the raw importance-sampling weights."""
        if slot is None:
            slot = DeviceBuffer(4 * self.N * batch)
        if n is None:
            n = DeviceBuffer(4 * self.N)
        if is_weight is None:
            is_weight = DeviceBuffer(4 * self.N * batch)
        nat.check(nat.lib().ofx_replay_sample_prioritized(self._h, seed, int(draw), int(batch), float(beta), slot.ptr, n.ptr,
                                                           is_weight.ptr))
        return slot, n, is_weight

    def replay_window_weights_into(self, is_weight, n_sampled, batch, first, max_rows, out):
        """The IS weights of replay_gather_valid's window (same arguments), packed and max-normalised into `out`."""
        nat.check(nat.lib().ofx_replay_window_weights(self._h, is_weight.ptr, n_sampled.ptr, int(batch), int(first),
                                                       int(max_rows), out.ptr))

    def replay_update_priorities(self, slot, n_sampled, batch, first, n_rows, rows_ptr, td_ptr):
        """Priority write-back for the n_rows gathered rows of that window from td [n_rows][2] = (e1, e2)."""
        nat.check(nat.lib().ofx_replay_update_priorities(self._h, slot.ptr, n_sampled.ptr, int(batch), int(first),
                                                          int(n_rows), rows_ptr, td_ptr))

    def replay_priorities(self, arena):
        """Masses (p^alpha) of one arena's rows, oldest first (the order of replay_rows)."""
        m = np.zeros(self.replay_capacity, np.float32)
        n = C.c_int32()
        nat.check(nat.lib().ofx_replay_priorities_host(self._h, int(arena), m.ctypes.data_as(C.c_void_p), C.byref(n)))
        return m[:n.value]

    # ------------------------------------------------------------ actor-side initial priorities (include/ofx.h: the contract)
    def policy_act(self, weights_ptr, epsilon, seed, tick=None, collecting=False, ship_mask_ptr=None, q_sa_ptr=None,
                   p_sp_ptr=None, v_act_ptr=None, v_ptr_ptr=None):
        """policy_forward + policy_explore in one call (the handle keeps iaction / ipointer, bit for bit those of the
        two calls), with the values of what was chosen into float32 [N][M] device arrays: q_sa = act_values[iaction],
        p_sp = the heat map at the chosen pointer, v_act = max(act_values), v_ptr = max(heat map).  None: kept by the
        handle for replay_capture_valued.  Does not synchronise."""
        nat.check(nat.lib().ofx_policy_act(self._h, weights_ptr, ship_mask_ptr, float(epsilon), seed,
                                           self.tick if tick is None else tick, int(bool(collecting)), q_sa_ptr, p_sp_ptr,
                                           v_act_ptr, v_ptr_ptr))

    def policy_act_boltzmann(self, weights_ptr, epsilon, tau_act, tau_ptr, seed, tick=None, collecting=False,
                             ship_mask_ptr=None, q_sa_ptr=None, p_sp_ptr=None, v_act_ptr=None, v_ptr_ptr=None):
        """policy_act with both heads sampled from softmax(Q / T) (opt-in Boltzmann exploration, include/ofx.h): arena a
        plays at T = tau * eps_a, eps_a the rate policy_explore would use (ladder included; a greedy arena stays greedy),
        on per-pixel Gumbel noise keyed by (seed, global arena, ship, tick).  `collecting`: exactly policy_act's
        collecting phase.  Results, values and the None rule are policy_act's.  Does not synchronise."""
        nat.check(nat.lib().ofx_policy_act_boltzmann(self._h, weights_ptr, ship_mask_ptr, float(epsilon), float(tau_act),
                                                     float(tau_ptr), seed, self.tick if tick is None else tick,
                                                     int(bool(collecting)), q_sa_ptr, p_sp_ptr, v_act_ptr, v_ptr_ptr))

    def policy_gumbel(self, words):
        """The sampling kernels' float32 Gumbel noise of the given Philox words (uint32 array), float32, same shape: a
        diagnostic of its accuracy against -log(-log1p(-(r + 0.5) / 2**32)) in float64."""
        w = np.ascontiguousarray(words, dtype=np.uint32)
        if w.size < 1:
            raise ValueError("ArenaBatch.policy_gumbel: at least one word expected")
        src, dst = DeviceBuffer(w.nbytes).upload(w), DeviceBuffer(4 * w.size)
        nat.check(nat.lib().ofx_policy_gumbel(self._h, src.ptr, int(w.size), dst.ptr))
        self.sync()
        return dst.download(np.float32, w.shape)

    def replay_actor_priorities(self, gamma):
        """Enable actor-side initial priorities on a prioritized memory: replay_capture_valued then gives every new
        row the mass of its one-step TD error under `gamma` instead of the arena's running maximum."""
        nat.check(nat.lib().ofx_replay_actor_priorities(self._h, float(gamma)))

    def replay_capture_valued(self, tick, ship_mask_ptr=None, iaction_ptr=None, ipointer_ptr=None, q_sa_ptr=None,
                              p_sp_ptr=None, v_act_ptr=None, v_ptr_ptr=None):
        """replay_capture with the values of this lock-step's choice (all four None: the handle's from the last
        policy_act, else all four given); call before step()."""
        nat.check(nat.lib().ofx_replay_capture_valued(self._h, int(tick), ship_mask_ptr, iaction_ptr, ipointer_ptr, q_sa_ptr,
                                                      p_sp_ptr, v_act_ptr, v_ptr_ptr))

    def replay_actor_values(self):
        """(q_sa, p_sp) of every ship's previous_*, float32 [N][M][2]: what a checkpoint carries next to the replay blob."""
        v = np.empty((self.N, self.M, 2), np.float32)
        nat.check(nat.lib().ofx_replay_actor_values_host(self._h, v.ctypes.data_as(C.c_void_p)))
        return v

    def set_replay_actor_values(self, values):
        a = np.asarray(values)
        if a.dtype != np.float32 or a.shape != (self.N, self.M, 2):
            raise ValueError("ArenaBatch.set_replay_actor_values: float32 [%d][%d][2] expected, got %s %s"
                             % (self.N, self.M, a.dtype, a.shape))
        a = np.ascontiguousarray(a)
        nat.check(nat.lib().ofx_replay_set_actor_values(self._h, a.ctypes.data_as(C.c_void_p)))

    # ------------------------------------------------------------ global minibatch sampling (include/ofx.h: the contract)
    def replay_sample_global(self, seed, draw, n_rows, prioritized=False, beta=0.0, arena=None, slot=None, is_weight=None):
        """n_rows rows from the union of all arenas' memories: uniform over rows without replacement, or (prioritized)
        stratified proportional to the masses across arenas -> (arena [n_rows], slot [n_rows], is_weight [n_rows] or
        None, n_drawn, eligible).  The first three are DeviceBuffers (the caller may hand them in), sorted by (arena,
        slot) with -1 / -1 / 0 after the n_drawn = min(n_rows, eligible) rows drawn; is_weight holds the IS weights
        over their maximum (uniform: 1.0 when a buffer is given, None otherwise).  Synchronises (two host integers)."""
        n_rows = int(n_rows)
        if arena is None:
            arena = DeviceBuffer(4 * n_rows)
        if slot is None:
            slot = DeviceBuffer(4 * n_rows)
        if is_weight is None and prioritized:
            is_weight = DeviceBuffer(4 * n_rows)
        n, elig = C.c_int32(0), C.c_int64(0)
        nat.check(nat.lib().ofx_replay_sample_global(self._h, seed, int(draw), n_rows, 1 if prioritized else 0, float(beta),
                                                      arena.ptr, slot.ptr, is_weight.ptr if is_weight is not None else None,
                                                      C.byref(n), C.byref(elig)))
        return arena, slot, is_weight, n.value, elig.value

    def replay_gather_list_into(self, arena, slot, n, rows, bits_prev, bits_next, nstep=1, gamma=0.0, ret=None, disc=None):
        """The n listed (arena, slot) rows into the caller's DeviceBuffers, one workgroup per row: what
        replay_gather_valid_into writes for them, or with ret / disc (float32 [n] DeviceBuffers) the n-step composites
        of replay_gather_nstep_into.  An entry that names no row becomes a padding row (ship = -1, zero maps).  Does not
        synchronise."""
        nat.check(nat.lib().ofx_replay_gather_list(self._h, arena.ptr, slot.ptr, int(n), int(nstep), float(gamma), rows.ptr,
                                                    bits_prev.ptr if bits_prev else None, bits_next.ptr if bits_next else None,
                                                    ret.ptr if ret else None, disc.ptr if disc else None))

    def replay_update_priorities_list(self, arena, slot, n, rows_ptr, td_ptr):
        """Priority write-back for the n rows of a gathered list from td [n][2] = (e1, e2); afterwards every arena's
        running maximum is the maximum over all arenas."""
        nat.check(nat.lib().ofx_replay_update_priorities_list(self._h, arena.ptr, slot.ptr, int(n), rows_ptr, td_ptr))

    # ------------------------------------------------------------ symmetry augmentation (include/ofx.h: the contract)
    def obs_transform(self, n_obs, op, bits, vec8=None, pointer=None):
        """Element op[i] (device uint8 [n_obs]; 0 .. 7, OFX_SYM_* bits) on observation i, in place: bits uint32
        [n_obs][2][W*H/32], and when given vec8 float32 [n_obs][8] and pointer int32 [n_obs][2] (DeviceBuffers).  An op
        above 7 leaves its observation untouched.  Does not synchronise."""
        nat.check(nat.lib().ofx_obs_transform(self._h, int(n_obs), op.ptr, bits.ptr, vec8.ptr if vec8 else None,
                                               pointer.ptr if pointer else None))

    def replay_augment_into(self, seed, draw, first, n, op_mask, rows, bits_prev, bits_next, op_out=None):
        """One element of op_mask per row of a gathered batch (Philox counter (arena_base, first + d, draw, stream 8)) on
        the row's two observations, heads and pointer, in place in the caller's DeviceBuffers; padding rows are left
        alone; op_out (device uint8 [n]) receives the elements.  op_mask == 1 launches nothing.  Does not synchronise."""
        nat.check(nat.lib().ofx_replay_augment(self._h, seed, int(draw), int(first), int(n), int(op_mask), rows.ptr,
                                                bits_prev.ptr, bits_next.ptr, op_out.ptr if op_out else None))

    # ------------------------------------------------------------ checkpoint (include/ofx.h: the blob's layout)
    def replay_export_bytes(self, arena0, n):
        """The exact size of the blob replay_export(arena0, n) returns (runs the device's count pass)."""
        v = C.c_size_t(0)
        nat.check(nat.lib().ofx_replay_export_bytes(self._h, int(arena0), int(n), C.byref(v)))
        return int(v.value)

    def replay_export(self, arena0, n):
        """The replay memory of local arenas [arena0, arena0 + n) as one self-describing blob (uint8 array): every
        state array raw, the frame ring packed on the device to (word index, word) pairs of its nonzero words."""
        blob = np.empty(self.replay_export_bytes(arena0, n), np.uint8)
        w = C.c_size_t(0)
        nat.check(nat.lib().ofx_replay_export(self._h, int(arena0), int(n), blob.ctypes.data_as(C.c_void_p), blob.nbytes,
                                               C.byref(w)))
        if w.value != blob.nbytes:
            raise Exception("replay_export: wrote %d of %d bytes" % (w.value, blob.nbytes))
        return blob

    def replay_import(self, arena0, n, blob):
        """Replace the memory of arenas [arena0, arena0 + n) by a replay_export blob; checked on the host
        (ofx_replay_blob_check) before anything is written, so a refused blob leaves the memory as it was."""
        blob = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview))
                                    else blob, np.uint8)
        nat.check(nat.lib().ofx_replay_import(self._h, int(arena0), int(n), blob.ctypes.data_as(C.c_void_p), blob.nbytes))

    STATE_FIELDS = ("ship_x", "ship_y", "ship_px", "ship_py", "ship_alive", "reward", "score", "n_lasers", "laser_x",
                    "laser_y", "laser_owner", "laser_dead", "killer", "time", "last_scores", "hull", "laser_dx", "laser_dy",
                    "obs_reward")          # the OFX_F_* fields by number: all of the arena state that outlives a lock-step

    def state_dict(self):
        """The arena state a resumed run needs: the 19 state fields as get() returns them, plus the episode and tick
        counters.  Not carried: the overflow counter (it counts "since the last call"), the episode sums (every restart
        rewrites them before they are read) and the observation maps (a pure function of the state)."""
        d = {name: self.get(f) for f, name in enumerate(self.STATE_FIELDS)}
        d["episode"], d["tick"] = int(self.episode), int(self.tick)
        return d

    def load_state_dict(self, d):
        """Upload state_dict()'s arrays into a spawned handle of the same shape and rasterise.  Every shape and dtype is
        checked before the first upload."""
        arrs = []
        for f, name in enumerate(self.STATE_FIELDS):
            if name not in d:
                raise ValueError("ArenaBatch.load_state_dict: field %r is missing" % name)
            a, dt = np.asarray(d[name]), np.dtype(_FIELD_DTYPE[f])
            nbytes = nat.lib().ofx_field_bytes(self._h, f)
            shape = (self.N,) if f in (nat.F_N_LASERS, nat.F_TIME) else (self.N, nbytes // dt.itemsize // self.N)
            if a.dtype != dt or a.shape != shape:
                raise ValueError("ArenaBatch.load_state_dict: field %r is %s %s, this batch holds %s %s"
                                 % (name, a.dtype, a.shape, dt, shape))
            arrs.append(np.ascontiguousarray(a))
        episode, tick = int(d["episode"]), int(d["tick"])
        self.sync()
        for f, a in enumerate(arrs):
            nat.check(nat.lib().ofx_memcpy_h2d(self.device_ptr(f), a.ctypes.data_as(C.c_void_p), a.nbytes))
        self.episode, self.tick = episode, tick
        self.rasterise()

    # ------------------------------------------------------------ n-step returns (include/ofx.h: the contract)
    def replay_gather_nstep_into(self, slot, n_sampled, batch, first, max_rows, nstep, gamma, rows, bits_prev, bits_next,
                                 ret, disc):
        """replay_gather_valid_into's window with every row the composite of its n-step chain: ret / disc [max_rows]
        float32 DeviceBuffers receive the discounted return and the bootstrap discount; returns n_rows."""
        n = C.c_int32()
        nat.check(nat.lib().ofx_replay_gather_nstep(self._h, slot.ptr, n_sampled.ptr, int(batch), int(first), int(max_rows),
                                                     int(nstep), float(gamma), rows.ptr, bits_prev.ptr if bits_prev else None,
                                                     bits_next.ptr if bits_next else None, ret.ptr, disc.ptr, C.byref(n)))
        return n.value

    def dqn_targets_nstep(self, weights_ptr, n, rows_ptr, bits_prev_ptr, bits_next_ptr, ret_ptr, disc_ptr, current=True):
        """dqn_targets with y = ret + disc * max(next_state) (ret / disc from replay_gather_nstep_into): host arrays q_sa,
        p_sp, y_act, y_ptr; current=False: only y_act, y_ptr."""
        n = int(n)
        bufs = [DeviceBuffer(4 * n) if (current or k >= 2) else None for k in range(4)]
        nat.check(nat.lib().ofx_dqn_targets_nstep(self._h, weights_ptr, n, rows_ptr, bits_prev_ptr, bits_next_ptr, ret_ptr,
                                                   disc_ptr, *[b.ptr if b else None for b in bufs]))
        self.sync()
        return tuple(b.download(np.float32, (n,)) if b else None for b in bufs)

    # ------------------------------------------- target network and Double DQN (include/ofx.h: the contract)
    def dqn_targets_double_into(self, online_ptr, target_ptr, n, rows_ptr, bits_prev_ptr, bits_next_ptr, gamma, y_act_ptr,
                                y_ptr_ptr, ret_ptr=None, disc_ptr=None, q_sa_ptr=None, p_sp_ptr=None):
        """Double DQN targets into the caller's device arrays: the online blob selects (iaction, ipointer) on next_state,
        the target blob evaluates them.  ret / disc (replay_gather_nstep_into) select the n-step form.  Does not
        synchronise."""
        nat.check(nat.lib().ofx_dqn_targets_double(self._h, online_ptr, target_ptr, int(n), rows_ptr, bits_prev_ptr,
                                                    bits_next_ptr, float(gamma), ret_ptr, disc_ptr, q_sa_ptr, p_sp_ptr,
                                                    y_act_ptr, y_ptr_ptr))

    def dqn_targets_into(self, weights_ptr, n, rows_ptr, bits_prev_ptr, bits_next_ptr, gamma, y_act_ptr, y_ptr_ptr,
                         ret_ptr=None, disc_ptr=None):
        """The plain targets into the caller's device arrays, bootstrapped from the blob at weights_ptr: y = r + gamma *
        max(next_state), or with ret / disc (replay_gather_nstep_into) y = ret + disc * max(next_state).  The current
        values q_sa / p_sp are not asked for.  Does not synchronise."""
        if ret_ptr is None:
            nat.check(nat.lib().ofx_dqn_targets(self._h, weights_ptr, n, rows_ptr, bits_prev_ptr, bits_next_ptr,
                                                 float(gamma), None, None, y_act_ptr, y_ptr_ptr))
        else:
            nat.check(nat.lib().ofx_dqn_targets_nstep(self._h, weights_ptr, n, rows_ptr, bits_prev_ptr, bits_next_ptr,
                                                       ret_ptr, disc_ptr, None, None, y_act_ptr, y_ptr_ptr))

    def policy_blend_weights(self, dst_buf, src_buf, tau):
        """dst = (1 - tau) * dst + tau * src over the whole weight blob (DeviceBuffers; tau = 1: a device copy) on the
        handle's stream: the soft / hard update of a target network.  Does not synchronise."""
        nat.check(nat.lib().ofx_policy_blend_weights(self._h, dst_buf.ptr, src_buf.ptr, float(tau)))

    def policy_forward_obs(self, weights_ptr, n_obs, bits_ptr, vec8_ptr, want_probe_ptr=None):
        """Forward on stored observations (Trainer.replay's predictions): host dict of act / iaction / ipointer /
        ptr_max (+ ptr_probe when want_probe_ptr, an int32 [n_obs][2] device array of (x, y), is given)."""
        n = int(n_obs)
        act, ia, ip, pm = DeviceBuffer(8 * n), DeviceBuffer(4 * n), DeviceBuffer(8 * n), DeviceBuffer(4 * n)
        pp = DeviceBuffer(4 * n) if want_probe_ptr else None
        nat.check(nat.lib().ofx_policy_forward_obs(self._h, weights_ptr, n, bits_ptr, vec8_ptr, act.ptr, ia.ptr, ip.ptr,
                                                    pm.ptr, want_probe_ptr, pp.ptr if pp else None))
        self.sync()
        out = {"act": act.download(np.float32, (n, 2)), "iaction": ia.download(np.int32, (n,)),
               "ipointer": ip.download(np.int32, (n, 2)), "ptr_max": pm.download(np.float32, (n,))}
        if pp:
            out["ptr_probe"] = pp.download(np.float32, (n,))
        return out

    # ------------------------------------------- soft and Munchausen targets (include/ofx.h: the contract)
    def policy_forward_obs_soft(self, weights_ptr, n_obs, bits_ptr, vec8_ptr, tau_ptr, want_probe_ptr=None, want_heat=False):
        """policy_forward_obs plus the soft value of the pointer head at temperature tau_ptr: the host dict gains ptr_soft
        = ptr_max + tau_ptr * ln(ptr_mass) and ptr_mass = sum exp((heat - ptr_max) / tau_ptr) (tau_ptr = 0: ptr_max and
        1), and with want_heat `heat`, the float32 [n_obs][H][W] map the sum was taken over."""
        n = int(n_obs)
        act, ia, ip, pm = DeviceBuffer(8 * n), DeviceBuffer(4 * n), DeviceBuffer(8 * n), DeviceBuffer(4 * n)
        ps, pz = DeviceBuffer(4 * n), DeviceBuffer(4 * n)
        pp = DeviceBuffer(4 * n) if want_probe_ptr else None
        heat = DeviceBuffer(4 * n * self.W * self.H) if want_heat else None
        nat.check(nat.lib().ofx_policy_forward_obs_soft(self._h, weights_ptr, n, bits_ptr, vec8_ptr, float(tau_ptr), act.ptr,
                                                         ia.ptr, ip.ptr, pm.ptr, want_probe_ptr, pp.ptr if pp else None,
                                                         ps.ptr, pz.ptr, heat.ptr if heat else None))
        self.sync()
        out = {"act": act.download(np.float32, (n, 2)), "iaction": ia.download(np.int32, (n,)),
               "ipointer": ip.download(np.int32, (n, 2)), "ptr_max": pm.download(np.float32, (n,)),
               "ptr_soft": ps.download(np.float32, (n,)), "ptr_mass": pz.download(np.float32, (n,))}
        if pp:
            out["ptr_probe"] = pp.download(np.float32, (n,))
        if heat:
            out["heat"] = heat.download(np.float32, (n, self.H, self.W))
        return out

    def dqn_targets_soft_into(self, weights_ptr, n, rows_ptr, bits_prev_ptr, bits_next_ptr, gamma, y_act_ptr, y_ptr_ptr,
                              tau_act, tau_ptr, m_alpha=0.0, m_clip=0.0, ret_ptr=None, disc_ptr=None, q_sa_ptr=None,
                              p_sp_ptr=None):
        """The soft targets into the caller's device arrays, bootstrapped from the blob at weights_ptr: dqn_targets_into
        with the maxima of next_state replaced by the soft values at (tau_act, tau_ptr); m_alpha > 0 adds the Munchausen
        term m_alpha * clamp(q - V(state), m_clip, 0) to the reward (one-step form only).  Does not synchronise."""
        nat.check(nat.lib().ofx_dqn_targets_soft(self._h, weights_ptr, int(n), rows_ptr, bits_prev_ptr, bits_next_ptr,
                                                  float(gamma), ret_ptr, disc_ptr, float(tau_act), float(tau_ptr),
                                                  float(m_alpha), float(m_clip), q_sa_ptr, p_sp_ptr, y_act_ptr, y_ptr_ptr))

    def dqn_targets(self, weights_ptr, n, rows_ptr, bits_prev_ptr, bits_next_ptr, gamma=0.9, current=True):
        """Trainer.replay's targets (qlearnIA_V2.py:251-270; gamma = 0.9, :51): host arrays q_sa, p_sp, y_act, y_ptr.
        current=False: only y_act, y_ptr (the forward on `state` is skipped; q_sa / p_sp come back as None)."""
        n = int(n)
        bufs = [DeviceBuffer(4 * n) if (current or k >= 2) else None for k in range(4)]
        nat.check(nat.lib().ofx_dqn_targets(self._h, weights_ptr, n, rows_ptr, bits_prev_ptr, bits_next_ptr, float(gamma),
                                             *[b.ptr if b else None for b in bufs]))
        self.sync()
        return tuple(b.download(np.float32, (n,)) if b else None for b in bufs)

    def dqn_fit(self, weights_buf, adam_m_buf, adam_v_buf, step, lr, n, rows_ptr, bits_prev_ptr, y_act_ptr, y_ptr_ptr,
                grad_buf=None):
        """One model.fit step of Trainer.replay on device (qlearnIA_V2.py:284); DeviceBuffers are updated in place.
        Returns (mse(output1), mse(output2))."""
        loss = (C.c_float * 2)()
        nat.check(nat.lib().ofx_dqn_fit(self._h, weights_buf.ptr, adam_m_buf.ptr, adam_v_buf.ptr, int(step), float(lr),
                                         int(n), rows_ptr, bits_prev_ptr, y_act_ptr, y_ptr_ptr,
                                         grad_buf.ptr if grad_buf else None, loss))
        return float(loss[0]), float(loss[1])

    def dqn_fit_weighted(self, weights_buf, adam_m_buf, adam_v_buf, step, lr, n, rows_ptr, bits_prev_ptr, y_act_ptr,
                         y_ptr_ptr, row_weight_ptr=None, td_ptr=None, grad_buf=None):
        """dqn_fit with per-row loss weights (Keras sample_weight) and the rows' (e1, e2) into td_ptr [n][2]; either may
        be None (no weights == dqn_fit).  Returns (loss1, loss2)."""
        loss = (C.c_float * 2)()
        nat.check(nat.lib().ofx_dqn_fit_weighted(self._h, weights_buf.ptr, adam_m_buf.ptr, adam_v_buf.ptr, int(step),
                                                  float(lr), int(n), rows_ptr, bits_prev_ptr, y_act_ptr, y_ptr_ptr,
                                                  grad_buf.ptr if grad_buf else None, loss, row_weight_ptr, td_ptr))
        return float(loss[0]), float(loss[1])

    def dqn_fit_robust(self, weights_buf, adam_m_buf, adam_v_buf, step, lr, n, rows_ptr, bits_prev_ptr, y_act_ptr,
                       y_ptr_ptr, huber_delta=0.0, clip_norm=0.0, row_weight_ptr=None, td_ptr=None, grad_buf=None):
        """dqn_fit_weighted under the Huber loss (huber_delta > 0: Keras Huber(delta), half the mse gradient inside the
        quadratic zone) and / or with the gradient clipped to a global norm of clip_norm before Adam (> 0:
        torch.nn.utils.clip_grad_norm_); 0 switches either off.  td_ptr receives the raw errors, grad_buf the gradient
        before scaling.  Returns (loss1, loss2, grad_norm): the Huber losses and the norm before clipping - None with both
        options off, where the call launches exactly what dqn_fit_weighted does."""
        loss, norm = (C.c_float * 2)(), C.c_float(0.0)
        on = bool(huber_delta) or bool(clip_norm)          # (NaN is true: it reaches the entry and is refused there)
        nat.check(nat.lib().ofx_dqn_fit_robust(self._h, weights_buf.ptr, adam_m_buf.ptr, adam_v_buf.ptr, int(step),
                                                float(lr), int(n), rows_ptr, bits_prev_ptr, y_act_ptr, y_ptr_ptr,
                                                grad_buf.ptr if grad_buf else None, loss, row_weight_ptr, td_ptr,
                                                float(huber_delta), float(clip_norm), C.byref(norm) if on else None))
        return float(loss[0]), float(loss[1]), (float(norm.value) if on else None)

    def dqn_acc_floats(self):
        """Floats of the accumulator between dqn_grad and dqn_apply: the weight blob's n_floats + the 256-float tail of
        batch statistics, losses and the micro-batch count (include/ofx.h, OFX_ACC_*)."""
        v = int(nat.lib().ofx_dqn_acc_floats(self._h))
        if v < 0:
            raise Exception("dqn_acc_floats: no policy layout")
        return v

    def dqn_grad(self, weights_buf, n, rows_ptr, bits_prev_ptr, y_act_ptr, y_ptr_ptr, acc_buf, reset, huber_delta=0.0,
                 row_weight_ptr=None, td_ptr=None, want_loss=False):
        """The gradient half of dqn_fit_robust: the n rows' gradient, batch statistics and losses go into acc_buf (a
        DeviceBuffer of 4 * dqn_acc_floats() bytes) - written with reset, added to it (plain fp32 adds, the count + 1)
        without.  Nothing of the weights or the Adam state is written.  td_ptr receives the raw errors.  Returns None and
        does not synchronise beyond the padding check, or with want_loss this micro-batch's (loss1, loss2)."""
        loss = (C.c_float * 2)() if want_loss else None
        nat.check(nat.lib().ofx_dqn_grad(self._h, weights_buf.ptr, int(n), rows_ptr, bits_prev_ptr, y_act_ptr, y_ptr_ptr,
                                          row_weight_ptr, td_ptr, float(huber_delta), acc_buf.ptr, 1 if reset else 0, loss))
        return (float(loss[0]), float(loss[1])) if want_loss else None

    def dqn_apply(self, weights_buf, adam_m_buf, adam_v_buf, step, lr, acc_buf, scale=1.0, clip_norm=0.0, want_norm=None):
        """The apply half: Adam, the moving statistics and the loss read-back on scale * acc_buf, the gradient clipped to a
        global norm of clip_norm (> 0) after scaling; DeviceBuffers are updated in place.  Returns (loss1, loss2,
        grad_norm): scale times the accumulated losses and the scaled norm before clipping - None unless clip_norm is set
        or want_norm asks for it.  dqn_grad(reset=True) + dqn_apply(scale=1) is dqn_fit_robust bit for bit."""
        loss, norm = (C.c_float * 2)(), C.c_float(0.0)
        on = bool(clip_norm) if want_norm is None else bool(want_norm)   # (NaN is true: refused at the entry)
        nat.check(nat.lib().ofx_dqn_apply(self._h, weights_buf.ptr, adam_m_buf.ptr, adam_v_buf.ptr, int(step), float(lr),
                                           acc_buf.ptr, float(scale), float(clip_norm), loss, C.byref(norm) if on else None))
        return float(loss[0]), float(loss[1]), (float(norm.value) if on else None)

    def dqn_fit_reference(self, weights_buf, adam_m_buf, adam_v_buf, step, lr, n, rows_ptr, bits_prev_ptr, bits_next_ptr,
                          gamma=0.9, grad_buf=None):
        """The fit step with Trainer.replay's quirks as written (qlearnIA_V2.py:251-285: whole-prediction targets,
        ptr_target[x][y], inputs = next_state); computes its own targets.  Returns (mse(output1), mse(output2))."""
        loss = (C.c_float * 2)()
        nat.check(nat.lib().ofx_dqn_fit_reference(self._h, weights_buf.ptr, adam_m_buf.ptr, adam_v_buf.ptr, int(step),
                                                   float(lr), int(n), rows_ptr, bits_prev_ptr, bits_next_ptr, float(gamma),
                                                   grad_buf.ptr if grad_buf else None, loss))
        return float(loss[0]), float(loss[1])

    # ------------------------------------------------------------ exploration ladder (include/ofx.h: the contract)
    def policy_epsilon_ladder(self, expo):
        """One exploration exponent per local arena (float64 [N]; ofighters_amd.exploration.apex_exponents): arena a then
        explores at epsilon ** expo[a] in policy_explore / policy_act, +inf = a greedy arena that never explores.  None
        removes the ladder.  Synchronises."""
        if expo is None:
            nat.check(nat.lib().ofx_policy_epsilon_ladder(self._h, None))
            return
        a = np.ascontiguousarray(expo, dtype=np.float64)
        if a.shape != (self.N,):
            raise ValueError("ArenaBatch.policy_epsilon_ladder: float64 [%d] expected, got shape %s" % (self.N, a.shape))
        nat.check(nat.lib().ofx_policy_epsilon_ladder(self._h, a.ctypes.data_as(C.c_void_p)))

    def policy_epsilon_ladder_host(self):
        """The exponents policy_epsilon_ladder set, float64 [N]; OfxError (OFX_ERR_STATE) while there is no ladder."""
        a = np.empty(self.N, np.float64)
        nat.check(nat.lib().ofx_policy_epsilon_ladder_host(self._h, a.ctypes.data_as(C.c_void_p)))
        return a

    def policy_explore(self, epsilon, seed, tick=None, collecting=False, ship_mask_ptr=None, iaction_ptr=None,
                       ipointer_ptr=None):
        """epsilon-greedy / collecting-phase random play over the last forward's results."""
        nat.check(nat.lib().ofx_policy_explore(self._h, float(epsilon), seed, self.tick if tick is None else tick,
                                               int(bool(collecting)), ship_mask_ptr, iaction_ptr, ipointer_ptr))

    # ------------------------------------------------------------ neuroevolution (include/ofx.h: the contract)
    def population_create(self, layers, P):
        """One population of P genomes of the scratch MLP `layers` ([8 + 2*W*H, ..., 4]) in HBM (ofx_population_create;
        ofighters_amd.evolution.Population owns these calls)."""
        l = np.ascontiguousarray(layers, dtype=np.int32)
        nat.check(nat.lib().ofx_population_create(self._h, l.ctypes.data_as(C.c_void_p), len(l), int(P)))

    def population_destroy(self):
        nat.check(nat.lib().ofx_population_destroy(self._h))

    def population_init(self, seed, generation=0):
        """U[-1, 1) on the fresh-genome stream for every element of every slot.  Does not synchronise."""
        nat.check(nat.lib().ofx_population_init(self._h, seed, int(generation)))

    def population_get(self, p, n_weights, n_biases):
        """Genome p as (weights float64 [n_weights], biases float64 [n_biases]) in the element order.  Synchronises."""
        (w, b), ptrs = _f64_out(n_weights, n_biases)
        nat.check(nat.lib().ofx_population_get(self._h, int(p), *ptrs))
        return w, b

    def population_set(self, p, weights, biases):
        _keep, ptrs = _f64_in(weights, biases)
        nat.check(nat.lib().ofx_population_set(self._h, int(p), *ptrs))

    def population_breed(self, plan, evolution_rate, mutation_rate, seed, generation):
        """Reproduction in place on the int32 [P] plan (kept / child of a kept slot / -1 fresh); the library checks the
        whole plan before it writes anything.  Does not synchronise."""
        pl = np.ascontiguousarray(plan, dtype=np.int32)
        nat.check(nat.lib().ofx_population_breed(self._h, pl.ctypes.data_as(C.c_void_p), float(evolution_rate),
                                                 float(mutation_rate), seed, int(generation)))

    def population_act(self, genome_of_ptr, out_ptr=None, y_ptr=None):
        """The forward with a genome per ship: overwrites, in the device action array (None = the batch's own, the one
        bot_actions wrote), the entries of the live ships whose entry of the device int32 [N][M] at genome_of_ptr names a
        genome; y_ptr: device float64 [N][M][4] or None.  Does not synchronise."""
        nat.check(nat.lib().ofx_population_act(self._h, genome_of_ptr, out_ptr or self._actions.ptr, y_ptr))

    def population_learn(self, genome_of_ptr, solution_ptr, rate, mask_ptr=None, out_ptr=None, y_ptr=None, err_ptr=None,
                         actions=True):
        """A gradient step per genome on its own ships (ofx_population_learn): the forward outputs of population_act
        from the weights before the call (actions into the batch's own array, or out_ptr; actions=False: none), then
        every genome's weights move by rate / n times its samples' gradients toward the device float64 [N][M][4] at
        solution_ptr.  mask_ptr: device uint8 [N][M] or None; err_ptr: device float64 [N][M] or None.  Does not
        synchronise."""
        out = (out_ptr or self._actions.ptr) if actions else None
        nat.check(nat.lib().ofx_population_learn(self._h, genome_of_ptr, solution_ptr, mask_ptr, float(rate), out, y_ptr,
                                                 err_ptr))

    def population_targets(self, solution_ptr, mask_ptr, teacher_ptr=None):
        """The teacher's actions (None = the batch's own array, as bot_actions wrote it) as targets float64 [N][M][4] and
        a mask uint8 [N][M] (ofx_population_targets).  Does not synchronise."""
        nat.check(nat.lib().ofx_population_targets(self._h, teacher_ptr or self._actions.ptr, solution_ptr, mask_ptr))

    def population_err_reduce(self, err_ptr, acc_ptr):
        """acc (device float64 [2]) += (sum, count) of the entries >= 0 of err (device float64 [N][M]), which are then
        set to -1 (ofx_population_err_reduce).  Does not synchronise."""
        nat.check(nat.lib().ofx_population_err_reduce(self._h, err_ptr, acc_ptr))

    def population_fitness(self, genome_of_ptr, sum_buf, count_buf, reset=False):
        """sum[g] (int64 [P]) += the score every ship flown by genome g banked at the last restart, count[g] (int32 [P])
        += 1 per such ship; reset zeroes both first.  Does not synchronise."""
        nat.check(nat.lib().ofx_population_fitness(self._h, genome_of_ptr, sum_buf.ptr, count_buf.ptr, int(bool(reset))))

    # ------------------------------------------------------------ evolution strategies (include/ofx.h: the contract)
    def es_create(self, layers):
        """One ES centre of the scratch MLP `layers` in HBM, beside any population (ofx_es_create; ofighters_amd.es.ES
        owns these calls)."""
        l = np.ascontiguousarray(layers, dtype=np.int32)
        nat.check(nat.lib().ofx_es_create(self._h, l.ctypes.data_as(C.c_void_p), len(l)))

    def es_destroy(self):
        nat.check(nat.lib().ofx_es_destroy(self._h))

    def es_init(self, seed, generation=0):
        """The centre becomes the fresh genome of slot 0 (stream 11).  Does not synchronise."""
        nat.check(nat.lib().ofx_es_init(self._h, seed, int(generation)))

    def es_get(self, n_weights, n_biases):
        """The centre as (weights float64 [n_weights], biases float64 [n_biases]) in the element order.  Synchronises."""
        (w, b), ptrs = _f64_out(n_weights, n_biases)
        nat.check(nat.lib().ofx_es_get(self._h, *ptrs))
        return w, b

    def es_set(self, weights, biases):
        _keep, ptrs = _f64_in(weights, biases)
        nat.check(nat.lib().ofx_es_set(self._h, *ptrs))

    def es_member(self, member, P, sigma, seed, generation, n_weights, n_biases):
        """Member `member` of P (P: the centre) at `generation`, materialised on the device, as (weights, biases) in the
        element order.  Synchronises."""
        (w, b), ptrs = _f64_out(n_weights, n_biases)
        nat.check(nat.lib().ofx_es_member(self._h, int(member), int(P), float(sigma), seed, int(generation), *ptrs))
        return w, b

    def es_act(self, member_of_ptr, P, sigma, seed, generation, out_ptr=None, y_ptr=None):
        """population_act with a member of the ES population per ship: the device int32 [N][M] at member_of_ptr holds
        values in [-1, P], P = the centre; the noise is regenerated in the kernel.  Does not synchronise."""
        nat.check(nat.lib().ofx_es_act(self._h, member_of_ptr, int(P), float(sigma), seed, int(generation),
                                       out_ptr or self._actions.ptr, y_ptr))

    def es_fitness(self, member_of_ptr, P, sum_buf, count_buf, reset=False):
        """population_fitness over members: sum int64 [P + 1], count int32 [P + 1], slot P the centre.  Does not
        synchronise."""
        nat.check(nat.lib().ofx_es_fitness(self._h, member_of_ptr, int(P), sum_buf.ptr, count_buf.ptr, int(bool(reset))))

    def es_requeue(self, member_of_ptr, queue_mask_ptr, P, total, queue_buf, sum_buf, count_buf, bank=True):
        """The member queue (ofx_es_requeue: the law, line by line): the ships of the arenas the last restart_finished /
        restart_arenas restarted bank to the member they flew (bank) and those under the device uint8 [N][M] at
        queue_mask_ptr take the next tickets of queue_buf (int64 [2]: next, completed), member = ticket % P, -1 once
        `total` tickets are out.  Rewrites the device int32 [N][M] at member_of_ptr.  Does not synchronise."""
        nat.check(nat.lib().ofx_es_requeue(self._h, member_of_ptr, queue_mask_ptr, int(P), int(total), queue_buf.ptr,
                                           sum_buf.ptr, count_buf.ptr, int(bool(bank))))

    def es_update(self, d, scale, seed, generation):
        """theta[e] += scale * sum_i d[i] * eps(i, e) in ascending pair order (ofx_es_update); d: float64 [P / 2].  Does
        not wait for the update."""
        (a,), (ptr,) = _f64_in(d)
        nat.check(nat.lib().ofx_es_update(self._h, ptr, a.shape[0], float(scale), seed, int(generation)))

    def es_opt_create(self):
        """The centre's optimiser state: the moments m and v, zeroed, in theta's layout (ofx_es_opt_create)."""
        nat.check(nat.lib().ofx_es_opt_create(self._h))

    def es_opt_destroy(self):
        nat.check(nat.lib().ofx_es_opt_destroy(self._h))

    def es_opt_get(self, n_weights, n_biases):
        """The moments as ((m weights, m biases), (v weights, v biases)) in the element order.  Synchronises."""
        out, ptrs = _f64_out(n_weights, n_biases, n_weights, n_biases)
        nat.check(nat.lib().ofx_es_opt_get(self._h, *ptrs))
        return (out[0], out[1]), (out[2], out[3])

    def es_opt_set(self, m_weights, m_biases, v_weights, v_biases):
        _keep, ptrs = _f64_in(m_weights, m_biases, v_weights, v_biases)
        nat.check(nat.lib().ofx_es_opt_set(self._h, *ptrs))

    def es_step(self, d, rule, gscale, decay, alpha, c1, k1, c2, k2, eps, seed, generation, stats_ptr=None):
        """The generation step through the optimiser (ofx_es_step: the law, line by line); d: float64 [P / 2], rule:
        nat.ES_RULE_MOMENTUM or nat.ES_RULE_ADAM, stats_ptr: device float64 [3] or None.  Does not wait for the step."""
        (a,), (ptr,) = _f64_in(d)
        nat.check(nat.lib().ofx_es_step(self._h, ptr, a.shape[0], int(rule), float(gscale),
                                        float(decay), float(alpha), float(c1), float(k1), float(c2), float(k2),
                                        float(eps), seed, int(generation), stats_ptr))

    # ------------------------------------------------------------ per-element adaptive sigma (ofx_es_sigma_*)
    def es_sigma_create(self, sigma0):
        """The centre's exploration width per element, every element sigma0, in theta's layout (ofx_es_sigma_create)."""
        nat.check(nat.lib().ofx_es_sigma_create(self._h, float(sigma0)))

    def es_sigma_destroy(self):
        nat.check(nat.lib().ofx_es_sigma_destroy(self._h))

    def es_sigma_get(self, n_weights, n_biases):
        """sigma as (weights float64 [n_weights], biases float64 [n_biases]) in the element order.  Synchronises."""
        (w, b), ptrs = _f64_out(n_weights, n_biases)
        nat.check(nat.lib().ofx_es_sigma_get(self._h, *ptrs))
        return w, b

    def es_sigma_set(self, weights, biases):
        _keep, ptrs = _f64_in(weights, biases)
        nat.check(nat.lib().ofx_es_sigma_set(self._h, *ptrs))

    def es_sigma_member(self, member, P, seed, generation, n_weights, n_biases):
        """es_member under the sigma vector: theta[e] + (+-sigma[e]) * eps(i, e).  Synchronises."""
        (w, b), ptrs = _f64_out(n_weights, n_biases)
        nat.check(nat.lib().ofx_es_sigma_member(self._h, int(member), int(P), seed, int(generation), *ptrs))
        return w, b

    def es_sigma_act(self, member_of_ptr, P, seed, generation, out_ptr=None, y_ptr=None):
        """es_act under the sigma vector.  Does not synchronise."""
        nat.check(nat.lib().ofx_es_sigma_act(self._h, member_of_ptr, int(P), seed, int(generation),
                                             out_ptr or self._actions.ptr, y_ptr))

    def es_sigma_step(self, d, s, rule, gscale, decay, alpha, c1, k1, c2, k2, eps, srate, smin, smax, seed, generation,
                      stats_ptr=None):
        """The generation step of the centre and of sigma in one pass (ofx_es_sigma_step: the law, line by line); d, s:
        float64 [P / 2], rule: nat.ES_RULE_PLAIN, _MOMENTUM or _ADAM, stats_ptr: device float64 [5] or None.  Does not
        wait for the step."""
        (a, w), ptrs = _f64_in(d, s)
        if a.ndim != 1 or a.shape != w.shape:
            raise ValueError("d and s are float64 [P / 2] arrays of one length, got %s and %s" % (a.shape, w.shape))
        nat.check(nat.lib().ofx_es_sigma_step(self._h, *ptrs,
                                              a.shape[0], int(rule), float(gscale), float(decay), float(alpha), float(c1),
                                              float(k1), float(c2), float(k2), float(eps), float(srate), float(smin),
                                              float(smax), seed, int(generation), stats_ptr))
