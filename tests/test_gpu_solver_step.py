"""ONE iteration of the solve on the device -- the step kernels, the resident and the streamed one-launch kernels -- against
the float64 reference of tests/solver_reference.py: the loss, the gradient as Adam's moments hold it, the Adam arithmetic
at t > 1 and the projection on the iteration.  The trajectory tests cannot see a gradient that is wrong by a positive
factor, a defect below 1e-5, or which iteration went wrong; these can.  The cases, the measures and where every bar comes
from: tests/solver_step_checks.py (shared with the host twin of this file, tests/test_solver_step_emulated.py).

Every figure (d_hip, d_ref, ratio; both measures; cold and warm) goes to solver_step.json in the directory RW_REPORT_DIR
names (default: test_reports/ at the repository's root, which git ignores)."""
import json
import os

import pytest

from tests import solver_step_checks as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_DIR = os.environ.get('RW_REPORT_DIR') or os.path.join(ROOT, 'test_reports')
REPORT = os.path.join(REPORT_DIR, 'solver_step.json')


def report(section, value):
    os.makedirs(REPORT_DIR, exist_ok=True)
    data = {}
    if os.path.isfile(REPORT):
        with open(REPORT) as f:
            data = json.load(f)
    data[section] = value
    with open(REPORT, 'w') as f:
        json.dump(data, f, indent=1, sort_keys=True)


@pytest.mark.parametrize('name', sorted(C.CASES, key=lambda n: (n[0], int(n[1:]))))
def test_one_iteration_against_float64(name, monkeypatch):
    """Cold, warm and (where the iteration projects) projected iteration of one case.  Admissibility -- no position within
    16 float32 deviations of the leaky ReLU's kink, and |out - val| >= 0.25 by construction -- is asserted before anything
    is launched; the kernel path is forced through the environment and asserted inside ``run`` (Solver.one_launch,
    hipsolve.LAST, and for one launch the crop copy only the streamed kernel is given)."""
    C.assert_admissible(name)
    C.set_path(monkeypatch, name)
    figures, failed = {}, {}
    for kind in C.kinds(name):
        fig, bad = C.evaluate(name, kind, C.run(name, kind, DEV))
        figures[kind] = fig
        print(name, kind, json.dumps(fig, sort_keys=True))
        if bad:
            failed[kind] = bad
    report(name, figures)
    assert not failed, (name, failed, figures)
