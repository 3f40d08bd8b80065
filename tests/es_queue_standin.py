"""The recording stand-ins ESRollout(auto_reset=True)'s CPU tests run against, in the style of tests/rollout_standin.py:
an engine and an ES that append every call to ONE shared log, so the order across the two is what the tests read.  A
helper module (not collected)."""
import numpy as np


class QueueEngine:
    """Logs the calls of a lock-step; nobody dies, nothing is simulated."""
    W = H = 400

    def __init__(self, log, N=4, M=3, arena_base=0):
        self.N, self.M, self.arena_base, self.log = N, M, arena_base, log
        self.episode = self.tick = 0
        self.auto = {"arena_episode": np.zeros(N, np.uint32), "dead_once": np.zeros((N, M), np.uint8)}

    def sync(self): pass
    def spawn_random(self, seed): self.log.append(("spawn",))
    def restart_random(self, seed):
        self.episode += 1
        self.log.append(("restart_random",))
    def episode_scores(self): return np.zeros(self.M + 1, np.int64)
    def restart_finished(self, seed, ship_mask_ptr=None, max_ticks=0):
        self.log.append(("restart_finished", ship_mask_ptr, max_ticks))
    def restart_arenas(self, seed, mask_buf=None): self.log.append(("restart_arenas", mask_buf))
    def bot_actions(self, beh, seed, tick=None): self.log.append(("bots", tick))
    def step(self):
        self.log.append(("step",))
        self.tick += 1
    def state_dict(self): return {"episode": self.episode, "tick": self.tick}
    def load_state_dict(self, d): self.episode, self.tick = d["episode"], d["tick"]
    def autoreset_state(self): return dict(self.auto, restarted=np.zeros(self.N, np.uint8))
    def load_autoreset_state(self, d):
        self.log.append(("load_autoreset",))
        self.auto = {k: np.array(d[k]) for k in ("arena_episode", "dead_once")}


class QueueES:
    """Logs ES's calls.  `done_at`: the polls (0-based, counted over the run) at which the queue reports
    completed == total; every other poll reports one evaluation short."""
    adaptive = False

    def __init__(self, log, done_at=()):
        self.log, self.done_at, self.polls = log, set(done_at), 0
        self.P = self.total = None
        self.member_of = None

    def assign(self, member_of, P):
        self.member_of, self.P = np.array(member_of), P
        self.log.append(("assign", self.member_of.copy(), P))
    def queue_begin(self, queue_mask, P, total):
        self.total = total
        self.log.append(("queue_begin", np.array(queue_mask), P, total))
    def requeue(self, bank=True): self.log.append(("requeue", bank))
    def queue_host(self):
        done = self.polls in self.done_at
        self.polls += 1
        self.log.append(("poll",))
        return (self.total, self.total if done else self.total - 1)
    def act(self, sigma, generation): self.log.append(("act", sigma, generation))
    def fitness(self, reset=False): self.log.append(("fitness", reset))
    def fitness_host(self):
        self.log.append(("fitness_host",))
        s, c = np.arange(self.P + 1, dtype=np.int64), np.ones(self.P + 1, np.int32)
        return s, c
    def update(self, d, lr, sigma, n_c, generation): self.log.append(("update", generation, n_c))
    def load_fitness(self, s, c): self.log.append(("load_fitness",))
    def member_of_host(self): return self.member_of.copy()
    def load_queue(self, member_of, queue): self.log.append(("load_queue", np.array(member_of), tuple(queue)))
