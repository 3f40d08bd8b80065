"""Record tests/golden/play_calls.json: every engine call TrainingRollout makes over the lock-steps of
tests/play_standin.py's cases, with the `boltzmann` option off.  The fixture pins the calls of the commit it was recorded
from, so record it from the commit BEFORE a change to the rollout, never from the code under test:

    python tests/record_play_calls.py [--package DIR] [--out FILE]

--package names the checkout whose `ofighters_amd` is recorded (default: this one); the stand-ins are this checkout's."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


class _Patch:
    def setattr(self, obj, name, value):
        setattr(obj, name, value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=os.path.dirname(HERE))
    ap.add_argument("--out", default=os.path.join(HERE, "golden", "play_calls.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    from tests import play_standin as st
    from tests.rollout_standin import fake_device_buffers
    sys.path.insert(0, os.path.abspath(args.package))
    import ofighters_amd.rollout as ro
    assert os.path.abspath(ro.__file__).startswith(os.path.abspath(args.package)), ro.__file__
    out = {name: st.run_case(ro, lambda: fake_device_buffers(_Patch()), tkw, rkw) for name, (tkw, rkw) in st.OFF_CASES.items()}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases, %d bytes -> %s" % (len(out), os.path.getsize(args.out), args.out))


if __name__ == "__main__":
    main()
