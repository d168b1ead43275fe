"""
oracle/check_golden.py -- TEST INFRASTRUCTURE.  Runs ONLY where oracle/gen_golden.py runs (it needs the reference project's source).

The committed fixtures are what oracle/gen_golden.py produces from the reference: regenerate ALL of them into a temporary folder (the whole
file, in order -- as `python oracle/gen_golden.py` does) and compare every array of every file bit for bit; then g14 once more by itself
(its generator seeds everything it draws: VERDICT r4 found it irreproducible).  Not part of the test suite, which stays within the
repository:  python oracle/check_golden.py      (exit code 0: every fixture reproduced)
"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _same(a, b):
    A, B = np.load(a), np.load(b)
    assert set(A.files) == set(B.files), (a, set(A.files) ^ set(B.files))
    bad = [k for k in A.files if not (A[k].dtype == B[k].dtype and A[k].shape == B[k].shape and A[k].tobytes() == B[k].tobytes())]
    assert not bad, (os.path.basename(a), bad[:8])


def _generate(out_dir, *names):
    env = dict(os.environ, US_GOLDEN_OUT=str(out_dir), PYTHONDONTWRITEBYTECODE="1", OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "8"))
    subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "gen_golden.py"), *names], check=True, env=env, stdout=subprocess.DEVNULL,
                   stderr=subprocess.PIPE, timeout=900)


def every_fixture_is_reproduced_by_the_committed_generator(tmp):
    _generate(tmp)
    committed = sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))
    assert len(committed) >= 14
    made = {os.path.basename(p) for p in glob.glob(os.path.join(tmp, "*.npz"))}
    assert made == {os.path.basename(p) for p in committed}
    for p in committed:
        _same(p, os.path.join(tmp, os.path.basename(p)))


def g14_does_not_depend_on_what_ran_before(tmp):
    _generate(tmp, "g14")
    for p in glob.glob(os.path.join(tmp, "*.npz")):
        _same(os.path.join(GOLDEN, os.path.basename(p)), p)


if __name__ == "__main__":
    for check in (every_fixture_is_reproduced_by_the_committed_generator, g14_does_not_depend_on_what_ran_before):
        with tempfile.TemporaryDirectory() as tmp:
            check(tmp)
        print(f"{check.__name__}: ok")
