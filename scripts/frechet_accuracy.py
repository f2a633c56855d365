"""Measures the numpy twin of the block Jacobi (tests/frechet_checks.py) against LAPACK and the truths, on the CPU:
every kind at every order and both block widths.  Writes the 'twin' part of profiles/frechet_accuracy.json and prints the
two tables tests/frechet_checks.py keeps (EIGEN_MARGIN, TWIN_DISTANCE_ERROR).  The 'device' part of the file is written by
tests/test_gpu_frechet.py when RW_FRECHET_RECORD names a path.

    python scripts/frechet_accuracy.py [--out profiles/frechet_accuracy.json]
"""
import argparse
import json
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import frechet_checks as C  # noqa: E402


def orders(b):
    return sorted(set([k * b for k in C.ORDERS_IN_B] + list(C.ORDERS)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frechet_accuracy.json'))
    args = ap.parse_args()
    rows, worst = [], 0.0
    for b in (8, 16):
        for n in orders(b):
            for kind in C.KINDS:
                mu1, s1, mu2, s2, exact = C.make_case(kind, n)
                lam, v, sweeps = C.eigh_twin(s1, b)
                res, orth = C.eigen_measures(s1, lam, v)
                lres, lorth, llam = C.lapack_measures(s1)
                top = llam.max()
                dlam = float(numpy.abs(numpy.sort(lam) - llam).max() / top) if top else float(numpy.abs(lam).max())
                # a LAPACK measure below one rounding (an exactly diagonalised input) counts as one rounding, as in the tests
                ratios = [x / max(y, C.EPS) for x, y in ((res, lres), (orth, lorth), (dlam, lres))]
                worst = max(worst, max(ratios))
                d2, (sw1, sw2) = C.frechet_twin(mu1, s1, mu2, s2, b)
                truth = C.distance_truth(mu1, s1, mu2, s2, exact)
                e = C.distance_error(d2, truth, s1, s2)
                rows.append(dict(case='%s-%d-b%d' % (kind, n, b), residual=res, orthogonality=orth, eigenvalues=dlam,
                                 lapack_residual=lres, lapack_orthogonality=lorth, ratios=ratios, eigh_sweeps=sweeps,
                                 distance_sweeps=[sw1, sw2], e_twin=e))
                print(rows[-1]['case'], 'ratios %.2f %.2f %.2f' % tuple(ratios), 'sweeps', sweeps, sw1, sw2, 'e_twin %.2e' % e,
                      flush=True)
    doc = {}
    if os.path.isfile(args.out):
        doc = json.load(open(args.out))
    doc['twin'] = dict(worst_ratio=worst, eigen_margin=2 * worst, cases=rows)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
    print('EIGEN_MARGIN = %r' % (2 * worst))
    print('TWIN_DISTANCE_ERROR = {')
    for r in rows:
        print("    %r: %.3e," % (r['case'], r['e_twin']))
    print('}')


if __name__ == '__main__':
    main()
