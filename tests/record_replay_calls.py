"""Record tests/golden/replay_calls.json: what DeviceTrainer.replay() issues on the stand-ins of tests/replay_standin.py
in every case of its table.  The fixture pins the calls of the commit it was recorded from, so record it from the commit
BEFORE a change to the trainer, never from the code under test:

    python tests/record_replay_calls.py [--package DIR] [--out FILE]

--package names the checkout whose `ofighters_amd` is recorded (default: this one); the stand-ins are always this
checkout's.  A trainer that still calls the library itself for the plain targets is recorded through the stand-in's shim
of `_native.lib` / `_native.check`."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=os.path.dirname(HERE))
    ap.add_argument("--out", default=os.path.join(HERE, "golden", "replay_calls.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    from tests import replay_standin as st
    sys.path.insert(0, os.path.abspath(args.package))
    import ofighters_amd.trainer as tr
    assert os.path.abspath(tr.__file__).startswith(os.path.abspath(args.package)), tr.__file__
    out = {name: st.run_case(tr, setattr, kw, hook, sched, bs) for name, kw, hook, sched, bs in st.cases()}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases, %d bytes -> %s" % (len(out), os.path.getsize(args.out), args.out))


if __name__ == "__main__":
    main()
