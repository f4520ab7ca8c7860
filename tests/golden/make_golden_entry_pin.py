"""Writes tests/golden/entry_sample_default.npz: the windows sample_trials / sample_trials_dm produce WITHOUT --sampler on seeded
checkpoints (tests/entry_pin_case.py).  The committed file was written on an MI355X by the commit before --sampler existed, so the test
that reads it pins the default (DDIM) output of the entry scripts byte for byte across that change.  Needs the GPU:

    python tests/golden/make_golden_entry_pin.py [output.npz]
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import entry_pin_case as E
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "entry_sample_default.npz")
    with tempfile.TemporaryDirectory() as out:
        paths = E.write_checkpoints(out)
        ldm = E.run_sample_trials(out, paths)
        dm = E.run_sample_trials_dm(out, paths)
        again = E.run_sample_trials(out, paths)
    assert ldm.tobytes() == again.tobytes(), "two runs of the same command differ: nothing to pin"
    assert np.isfinite(ldm).all() and np.isfinite(dm).all()
    np.savez(dst, sample_trials=ldm, sample_trials_dm=dm)
    print(f"wrote {dst}: sample_trials {ldm.shape} rms {float(np.sqrt((ldm ** 2).mean())):.4f}, sample_trials_dm {dm.shape} rms "
          f"{float(np.sqrt((dm ** 2).mean())):.4f}")


if __name__ == "__main__":
    main()
