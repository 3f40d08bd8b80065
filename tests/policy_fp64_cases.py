"""What the comparisons of the policy forward against float64 (tests/policy_ref64.py) share: the bounds, the report
file and the seeded rollout.  A helper module (not collected)."""
import json
import os

# max |err| / max |value| of a tensor against float64.  Measured (r02, gpurun_out/policy_fp64_report.json):
#   HIP path      act 3.6e-6 (4096 x 8, bench weights), heat interior 5.8e-7, heat frame 5.9e-7
#   C restatement act 2.0e-6,                           heat interior 2.0e-6, heat frame 1.9e-6
# arg-max equal to the float64 map's for 288 of 288 ships.
TOL_ACT, TOL_HEAT, TOL_FRAME = 1.5e-5, 8e-6, 8e-6
REPORT = os.path.join(os.path.dirname(__file__), "..", "gpurun_out", "policy_fp64_report.json")


def rollout(N, M, seed, ticks):
    from ofighters_amd import ArenaBatch
    b = ArenaBatch(N, M)
    b.spawn_random(seed)
    for t in range(ticks):
        b.bot_actions(["turret"] * (M // 2) + ["random"] * (M - M // 2), seed, tick=t)
        b.step(actions_ptr=b._actions.ptr)
    return b


def report(tag, rec):
    try:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        data = json.load(open(REPORT)) if os.path.exists(REPORT) else {}
        data[tag] = rec
        json.dump(data, open(REPORT, "w"), indent=1)
    except OSError:
        pass
    print(tag, rec)
