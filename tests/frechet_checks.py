"""Inputs, truths, the numpy twin and the measured margins of the device Frechet route (rw_frechet.hip,
hip.eigh_psd_f64, samples.frechet_distance(device=...)).

The twin restates the block algorithm of rw_frechet.hip in numpy -- the same padding, the same round-robin ordering of
the blocks and of the pairs inside a block pair, the same tolerance and noise floor, the same bounded inner solve -- with
numpy's summation order in place of the MFMA's.  It says what the ALGORITHM costs in accuracy; the device is held to a
small multiple of that (the margins at the end of this file, measured by scripts/frechet_accuracy.py and recorded with
every ratio in profiles/frechet_accuracy.json).
"""
import numpy

EPS = 2.0 ** -52
MAX_INNER = 10            # RW_JACOBI_INNER_SWEEPS
MAX_SWEEPS = 40           # hip.JACOBI_MAX_SWEEPS
ORDERS_IN_B = (2, 4, 6)   # 2b: one pair, only the inner solve; 4b; 6b
ORDERS = (70, 160, 256)   # 70: padding and (9 blocks of 8, 5 of 16) a bye
KINDS = ('decay', 'rankdef', 'span13', 'commute', 'diagonal', 'same', 'zero', 'repeat')


def padded_order(n, b):
    """The order the kernels run at: a multiple of the block width, at least one block pair."""
    return max(2 * b, -(-n // b) * b)


def thresholds(n_pad):
    """(tol, floor): RW_JACOBI_TOL / RW_JACOBI_FLOOR of include/rewriting_hip.h.  A dot product of n_pad terms carries a
    rounding error of at most n_pad eps |x||y|: a cosine below that is not known to differ from zero.  A column that
    rounding alone can produce from the largest one has a norm of that size relative to it."""
    return n_pad * EPS, n_pad * EPS


def circle_pair(count, r, k):
    """Pair k of round r of the circle method over ``count`` players: (lo, hi), or None for a bye (odd count, the player
    that meets the dummy)."""
    m = count + (count & 1)
    if k == 0:
        i, j = m - 1, r
    else:
        i, j = (r + k) % (m - 1), (r - k) % (m - 1)
    if i > j:
        i, j = j, i
    return None if j >= count else (i, j)


def schedule(count):
    """The steps of one sweep: a list (one entry per launch) of lists of block pairs."""
    m = count + (count & 1)
    return [[p for p in (circle_pair(count, r, k) for k in range(m // 2)) if p is not None] for r in range(m - 1)]


def _rotate(a, p, q, c, s, axis):
    if axis == 2:
        ap, aq = a[:, :, p].copy(), a[:, :, q].copy()
        a[:, :, p] = c[:, None, :] * ap - s[:, None, :] * aq
        a[:, :, q] = s[:, None, :] * ap + c[:, None, :] * aq
    else:
        ap, aq = a[:, p, :].copy(), a[:, q, :].copy()
        a[:, p, :] = c[:, :, None] * ap - s[:, :, None] * aq
        a[:, q, :] = s[:, :, None] * ap + c[:, :, None] * aq


def inner_solve(a, ref2, tol, floor):
    """Cyclic two-sided Jacobi on the batch of Gram matrices a (P, W, W), rotations accumulated from the identity, then
    the columns of Q ordered by decreasing diagonal of Q^T a Q (ties: the lower index first).
    Returns (Q, rotations per matrix, True where the order changed)."""
    npair, w, _ = a.shape
    a = a.copy()
    q_acc = numpy.tile(numpy.eye(w), (npair, 1, 1))
    count = numpy.zeros(npair, dtype=numpy.int64)
    rounds = [[circle_pair(w, r, k) for k in range(w // 2)] for r in range(w - 1)]
    with numpy.errstate(all='ignore'):
        for _ in range(MAX_INNER):
            live = numpy.zeros(npair, dtype=numpy.int64)
            for pairs in rounds:
                p = numpy.array([x[0] for x in pairs])
                q = numpy.array([x[1] for x in pairs])
                app, aqq, apq = a[:, p, p], a[:, q, q], a[:, p, q]
                thr = tol * numpy.sqrt(numpy.maximum(app, 0.0)) * numpy.sqrt(numpy.maximum(aqq, 0.0))
                do = (numpy.abs(apq) > thr) & (numpy.maximum(app, aqq) > (floor * floor) * ref2)
                zeta = (aqq - app) / (2.0 * apq)
                t = numpy.copysign(1.0, zeta) / (numpy.abs(zeta) + numpy.sqrt(1.0 + zeta * zeta))
                c = 1.0 / numpy.sqrt(1.0 + t * t)
                s = c * t
                c, s = numpy.where(do, c, 1.0), numpy.where(do, s, 0.0)
                _rotate(a, p, q, c, s, 2)
                _rotate(q_acc, p, q, c, s, 2)
                _rotate(a, p, q, c, s, 1)
                live += do.sum(1)
            count += live
            if not live.any():
                break
    order = numpy.argsort(-numpy.diagonal(a, axis1=1, axis2=2), axis=1, kind='stable')
    q_acc = numpy.take_along_axis(q_acc, order[:, None, :], axis=2)
    return q_acc, count, (order != numpy.arange(w)).any(1)


def eigh_twin(s, b, vectors=True, max_sweeps=MAX_SWEEPS):
    """(eigenvalues, eigenvectors as columns or None, sweeps) of a symmetric PSD matrix by the block one-sided Jacobi of
    rw_frechet.hip; the eigenvalues are in the kernels' order with vectors, ascending without.  Row j of the working
    arrays is column j of G and of V."""
    s = numpy.asarray(s, dtype=numpy.float64)
    n = s.shape[0]
    npad = padded_order(n, b)
    g = numpy.zeros((npad, npad))
    g[:n, :n] = s
    if not numpy.isfinite(g).all():
        raise ValueError('non-finite input')
    v = numpy.eye(npad) if vectors else None
    tol, floor = thresholds(npad)
    ref2 = (g * g).sum(1).max()
    steps = schedule(npad // b)
    for sweep in range(1, max_sweeps + 1):
        total = 0
        for pairs in steps:
            rows = numpy.array([list(range(i * b, i * b + b)) + list(range(j * b, j * b + b)) for i, j in pairs])
            p = g[rows]                                     # (P, 2b, npad)
            gram = p @ p.transpose(0, 2, 1)
            q_acc, count, moved = inner_solve(gram, ref2, tol, floor)
            total += int(count.sum())
            hit = (count > 0) | moved
            if hit.any():
                qt = q_acc[hit].transpose(0, 2, 1)
                g[rows[hit]] = qt @ p[hit]
                if vectors:
                    v[rows[hit]] = qt @ v[rows[hit]]
        if total == 0:
            lam = numpy.sqrt((g * g).sum(1))
            if not vectors:
                return numpy.sort(lam)[npad - n:], None, sweep
            keep = ~(v[:, n:] != 0).any(1)                  # the padding's columns are unit vectors past row n, still
            return lam[keep], v[keep, :n].T.copy(), sweep
    raise RuntimeError('no convergence in %d sweeps' % max_sweeps)


def frechet_twin(mu1, s1, mu2, s2, b):
    """(d^2, sweeps of the two solves) by the device route's steps: eigh(S1) -> B = F^T S2 F -> eigenvalues -> d^2."""
    n = s1.shape[0]
    npad = padded_order(n, b)
    p1, p2 = numpy.zeros((npad, npad)), numpy.zeros((npad, npad))
    p1[:n, :n], p2[:n, :n] = s1, s2
    lam, v, sw1 = eigh_twin(p1, b, vectors=True)
    root = numpy.sqrt(lam)
    t = (root[:, None] * v.T) @ p2
    bmat = (t @ v) * root[None, :]
    mu, _, sw2 = eigh_twin(bmat, b, vectors=False)
    diff = mu1 - mu2
    return float(diff.dot(diff) + numpy.trace(s1) + numpy.trace(s2) - 2.0 * numpy.sqrt(mu).sum()), (sw1, sw2)


# ------------------------------------------------------------------ inputs and truths
def _orthogonal(rng, n):
    q, r = numpy.linalg.qr(rng.standard_normal((n, n)))
    return q * numpy.sign(numpy.diag(r))


def _spd(q, d):
    s = (q * d) @ q.T
    return (s + s.T) / 2


def make_case(kind, n, seed=0):
    """(mu1, S1, mu2, S2, analytic Tr sqrt(S1 S2) or None)."""
    rng = numpy.random.RandomState(1000 * seed + n)
    # |mu1 - mu2|^2 of the order of the traces: the error measure is relative to them
    mu1, mu2 = rng.standard_normal(n) / numpy.sqrt(n), rng.standard_normal(n) / numpy.sqrt(n)
    decay = 1.0 / (1.0 + numpy.arange(n)) ** 2
    exact = None
    if kind == 'decay':
        s1, s2 = _spd(_orthogonal(rng, n), decay), _spd(_orthogonal(rng, n), decay[::-1] + 0.01)
    elif kind == 'rankdef':
        k = max(2, n // 4)
        s1 = numpy.cov(rng.standard_normal((k, n)) * (1 + numpy.arange(n) % 7), rowvar=False)
        s2 = numpy.cov(rng.standard_normal((k, n)) + 0.3 * rng.standard_normal((k, 1)), rowvar=False)
    elif kind == 'span13':
        s1 = _spd(_orthogonal(rng, n), numpy.logspace(0, -13, n))
        s2 = _spd(_orthogonal(rng, n), numpy.logspace(-13, 0, n))
    elif kind == 'commute':
        q = _orthogonal(rng, n)
        d1, d2 = rng.uniform(0.1, 2.0, n), rng.uniform(0.1, 2.0, n)
        d1[rng.permutation(n)[:(3 * n) // 10]] = 0.0
        d2[rng.permutation(n)[:(3 * n) // 10]] = 0.0
        s1, s2 = _spd(q, d1), _spd(q, d2)
        exact = float(numpy.sqrt(d1 * d2).sum())
    elif kind == 'diagonal':
        d1, d2 = rng.uniform(0.0, 2.0, n), rng.uniform(0.0, 2.0, n)
        s1, s2 = numpy.diag(d1), numpy.diag(d2)
        exact = float(numpy.sqrt(d1 * d2).sum())
    elif kind == 'same':
        s1 = _spd(_orthogonal(rng, n), decay)
        s2 = s1.copy()
        exact = float(numpy.trace(s1))
    elif kind == 'zero':
        s1 = numpy.zeros((n, n))
        s2 = _spd(_orthogonal(rng, n), decay)
        exact = 0.0
    elif kind == 'repeat':
        s1 = numpy.diag(rng.uniform(0.5, 2.0, n))
        s1[:2, :2] = 1.0                                    # [[1, 1], [1, 1]]: equal norms, zeta = 0
        s2 = _spd(_orthogonal(rng, n), decay)
    else:
        raise KeyError(kind)
    return mu1, s1, mu2, s2, exact


def distance_truth(mu1, s1, mu2, s2, exact=None):
    """d^2 with Tr sqrt(S1 S2) analytic where the pair commutes, else by LAPACK's eigh in float64: the eigenvalues of
    F^T S2 F, F = V sqrt(lambda), negative roundings clipped."""
    if exact is None:
        lam, v = numpy.linalg.eigh(s1)
        f = v * numpy.sqrt(numpy.maximum(lam, 0.0))
        mu = numpy.linalg.eigvalsh(f.T @ s2 @ f)
        exact = numpy.sqrt(numpy.maximum(mu, 0.0)).sum()
    diff = mu1 - mu2
    return float(diff.dot(diff) + numpy.trace(s1) + numpy.trace(s2) - 2.0 * exact)


def distance_error(d2, truth, s1, s2):
    return abs(d2 - truth) / (numpy.trace(s1) + numpy.trace(s2))


def eigen_measures(s, lam, v):
    """(||S V - V L||_F / ||S||_F, ||V^T V - I||_F); a zero matrix has residual measure ||S V - V L||_F itself."""
    norm = numpy.linalg.norm(s)
    res = numpy.linalg.norm(s @ v - v * lam[None, :])
    return res / norm if norm else res, numpy.linalg.norm(v.T @ v - numpy.eye(s.shape[0]))


def lapack_measures(s):
    lam, v = numpy.linalg.eigh(s)
    return eigen_measures(s, lam, v) + (lam,)


# ------------------------------------------------------------------ the measured margins
# scripts/frechet_accuracy.py on the CPU, every kind at every order above and both block widths
# (profiles/frechet_accuracy.json holds each ratio).  EIGEN_MARGIN is twice the twin's worst ratio to LAPACK's own measure
# on the same matrix (residual, orthogonality, eigenvalue difference / lambda_max against LAPACK's residual measure).
EIGEN_MARGIN = 788.8            # 2 x 394.41 (span13-256-b8)
# e_twin by '<kind>-<order>-b<block>': |d^2 - truth| / (Tr S1 + Tr S2) of frechet_twin
TWIN_DISTANCE_ERROR = {
    'decay-16-b8': 2.001e-15,
    'rankdef-16-b8': 1.306e-09,
    'span13-16-b8': 2.244e-10,
    'commute-16-b8': 3.391e-09,
    'diagonal-16-b8': 0.000e+00,
    'same-16-b8': 1.261e-15,
    'zero-16-b8': 0.000e+00,
    'repeat-16-b8': 1.934e-16,
    'decay-32-b8': 8.010e-15,
    'rankdef-32-b8': 1.265e-09,
    'span13-32-b8': 2.099e-08,
    'commute-32-b8': 6.426e-09,
    'diagonal-32-b8': 1.124e-16,
    'same-32-b8': 1.279e-14,
    'zero-32-b8': 0.000e+00,
    'repeat-32-b8': 1.033e-15,
    'decay-48-b8': 1.191e-14,
    'rankdef-48-b8': 1.765e-09,
    'span13-48-b8': 3.074e-08,
    'commute-48-b8': 8.796e-09,
    'diagonal-48-b8': 0.000e+00,
    'same-48-b8': 1.941e-14,
    'zero-48-b8': 0.000e+00,
    'repeat-48-b8': 1.295e-15,
    'decay-70-b8': 1.726e-14,
    'rankdef-70-b8': 2.875e-09,
    'span13-70-b8': 4.707e-08,
    'commute-70-b8': 8.773e-09,
    'diagonal-70-b8': 0.000e+00,
    'same-70-b8': 2.669e-14,
    'zero-70-b8': 0.000e+00,
    'repeat-70-b8': 1.850e-15,
    'decay-160-b8': 4.316e-14,
    'rankdef-160-b8': 1.657e-09,
    'span13-160-b8': 7.743e-08,
    'commute-160-b8': 1.178e-08,
    'diagonal-160-b8': 1.763e-16,
    'same-160-b8': 7.127e-14,
    'zero-160-b8': 0.000e+00,
    'repeat-160-b8': 2.489e-15,
    'decay-256-b8': 6.963e-14,
    'rankdef-256-b8': 1.555e-09,
    'span13-256-b8': 1.237e-07,
    'commute-256-b8': 1.467e-08,
    'diagonal-256-b8': 1.124e-16,
    'same-256-b8': 1.053e-13,
    'zero-256-b8': 0.000e+00,
    'repeat-256-b8': 3.097e-15,
    'decay-32-b16': 2.503e-15,
    'rankdef-32-b16': 1.265e-09,
    'span13-32-b16': 2.324e-08,
    'commute-32-b16': 6.055e-09,
    'diagonal-32-b16': 1.124e-16,
    'same-32-b16': 5.365e-15,
    'zero-32-b16': 0.000e+00,
    'repeat-32-b16': 5.166e-16,
    'decay-64-b16': 1.526e-14,
    'rankdef-64-b16': 6.541e-10,
    'span13-64-b16': 4.026e-08,
    'commute-64-b16': 7.079e-09,
    'diagonal-64-b16': 1.120e-16,
    'same-64-b16': 2.807e-14,
    'zero-64-b16': 0.000e+00,
    'repeat-64-b16': 1.249e-15,
    'decay-70-b16': 1.412e-14,
    'rankdef-70-b16': 2.875e-09,
    'span13-70-b16': 3.289e-08,
    'commute-70-b16': 8.388e-09,
    'diagonal-70-b16': 0.000e+00,
    'same-70-b16': 2.356e-14,
    'zero-70-b16': 0.000e+00,
    'repeat-70-b16': 1.514e-15,
    'decay-96-b16': 2.142e-14,
    'rankdef-96-b16': 1.637e-09,
    'span13-96-b16': 4.426e-08,
    'commute-96-b16': 1.051e-08,
    'diagonal-96-b16': 1.418e-16,
    'same-96-b16': 3.994e-14,
    'zero-96-b16': 0.000e+00,
    'repeat-96-b16': 1.786e-15,
    'decay-160-b16': 3.642e-14,
    'rankdef-160-b16': 1.660e-09,
    'span13-160-b16': 1.025e-07,
    'commute-160-b16': 1.117e-08,
    'diagonal-160-b16': 1.763e-16,
    'same-160-b16': 6.301e-14,
    'zero-160-b16': 0.000e+00,
    'repeat-160-b16': 2.212e-15,
    'decay-256-b16': 5.853e-14,
    'rankdef-256-b16': 1.555e-09,
    'span13-256-b16': 1.421e-07,
    'commute-256-b16': 1.391e-08,
    'diagonal-256-b16': 1.124e-16,
    'same-256-b16': 8.998e-14,
    'zero-256-b16': 0.000e+00,
    'repeat-256-b16': 2.551e-15,
}
