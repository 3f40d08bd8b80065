"""Shared helpers to replay tests/golden/step_*.npz traces (recorded from the
live reference by oracle/gen_golden.py) through an engine and compare."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def step_traces():
    return sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GOLDEN, "step_*.npz")))


def load_trace(name):
    z = np.load(os.path.join(GOLDEN, "step_%s.npz" % name))
    return {k: z[k] for k in z.files}


def unpack_map(bits, w=400, h=400):
    return np.unpackbits(bits)[: w * h].reshape(w, h)


CONSTANTS = ("ship_radius", "laser_radius", "ship_speed", "laser_speed",
             "reward_death", "reward_kill", "reward_aim", "reward_trajectory")


def trace_constants(z):
    """The game constants a trace was recorded at, as config keywords: the const_* entries of the step_const_* traces
    (oracle/gen_golden.py const_traces); empty for the traces recorded at the reference's own numbers."""
    return {k: int(z["const_" + k]) for k in CONSTANTS if "const_" + k in z}
