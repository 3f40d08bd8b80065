#!/opt/conda/bin/python3.9
"""Golden vectors of the scratch network's learning step (TEST INFRASTRUCTURE, run where oracle/gen_golden.py runs and
with its interpreter): imports the live reference's Neural_network and records, for the nets [24, 5, 4], [72, 9, 4] and
[72, 13, 7, 4] on observations with a binary tail,

    weights before, observations, solutions
    backprop's gradients of every observation                       (agents/neural_network.py:338-393)
    weights after update_network on the first 1, 2 and 5            (:241-300)
    weights after update_network_continuous(obs 0, sol 0, 0.01)     (:319-334)

into tests/golden/scratch_backprop.npz.  Only data is written.  update_network_continuous multiplies the LIST of
per-layer gradients by the rate in one np.multiply, which newer numpy refuses for layers of different shapes; where
it raises, `cont_ok_<tag>` is 0 and no such weights are stored.
Usage:  /opt/conda/bin/python3.9 tools/gen_learn_golden.py [outdir]
"""
import contextlib
import copy
import io
import os
import sys

sys.dont_write_bytecode = True
from unittest.mock import MagicMock

for _m in ["keras", "keras.models", "keras.layers", "keras.layers.core", "keras.optimizers",
           "keras.layers.advanced_activations", "keras.backend", "tensorflow"]:
    sys.modules[_m] = MagicMock()
sys.path.insert(0, "/root/reference")

import numpy as np

with contextlib.redirect_stdout(io.StringIO()):
    from ofighters.agents.neural_network import Neural_network

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests",
                                                         "golden")


def flat(nn):
    return np.concatenate([w.ravel() for w in nn.weights_layers] + [b.ravel() for b in nn.biases_layers])


def main():
    out = {}
    for tag, layers, seed in (("a", [24, 5, 4], 0), ("b", [72, 9, 4], 1), ("c", [72, 13, 7, 4], 2)):
        np.random.seed(seed)
        nn = Neural_network(list(layers))
        rs = np.random.RandomState(2000 + seed)
        n_obs = 5
        X = np.concatenate([rs.uniform(-2, 2, (n_obs, 8)), (rs.rand(n_obs, layers[0] - 8) < 0.2).astype(np.float64)], 1)
        S = rs.uniform(0, 1, (n_obs, 4))
        out["layers_" + tag] = np.array(layers, np.int32)
        out["before_" + tag] = flat(nn)
        out["x_" + tag], out["sol_" + tag] = X, S
        obs = [x.reshape(-1, 1) for x in X]
        sol = [s.reshape(-1, 1) for s in S]
        grads = []
        for x, s in zip(obs, sol):
            gw, gb = nn.backprop(x, s - nn.feed(x))
            grads.append(np.concatenate([w.ravel() for w in gw] + [b.ravel() for b in gb]))
        out["grad_" + tag] = np.stack(grads)
        with contextlib.redirect_stdout(io.StringIO()):
            for n in (1, 2, 5):
                m = copy.deepcopy(nn)
                m.update_network(obs[:n], sol[:n])
                out["after%d_%s" % (n, tag)] = flat(m)
        m = copy.deepcopy(nn)
        try:
            m.update_network_continuous(obs[0], sol[0], 0.01)
            out["cont_" + tag] = flat(m)
            out["cont_ok_" + tag] = np.int32(1)
        except ValueError as e:
            out["cont_ok_" + tag] = np.int32(0)
            print("update_network_continuous on %s: %s" % (layers, e))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "scratch_backprop.npz"), **out)
    print("scratch_backprop:", {k: v.shape for k, v in out.items()})


main()
