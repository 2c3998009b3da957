"""CPU: the pieces the three refiners share (prediction/refinement.py) — that the four public step / sigma functions are still what
their own bodies were before they delegated, that the shared Levenberg loop accepts exactly the strict decreases, and that
BundleRefiner(silhouette=0) solves on the depth words as the kernel wrote them.  The stub engine and the host-only tensors are
tests/test_silhouette_host.py's."""
import numpy as np
import pytest

from rope_s3d_amd.prediction import refinement as rf

from test_silhouette_host import ANGLES, DEPTH, POSE, StubEngine, _intr, on_the_host  # noqa: F401  (on_the_host is a fixture)


# ---------------------------------------------------------------------------------------------- (a) step and sigma
# The bodies as they stood before the four functions shared one: restated here word for word, each with its own solve.
def _old_unpack(words, slots):
    A = np.zeros((slots, slots))
    if slots == 6:
        A[np.triu_indices(6)] = words[10:31]
        return A + np.triu(A, 1).T, np.array(words[4:10], np.float64)
    A[np.triu_indices(12)] = words[16:94]
    return A + np.triu(A, 1).T, np.array(words[4:16], np.float64)


def _old_solve_finite(M, rhs):
    try:
        x = np.linalg.solve(M, rhs)
    except np.linalg.LinAlgError:
        return None
    return x if np.isfinite(x).all() else None


def old_levenberg_step(words, active, lam):
    A, g = _old_unpack(words, 6)
    idx = [j for j in active if A[j, j] > 0]
    d = np.zeros(6)
    if not idx:
        return d
    S = A[np.ix_(idx, idx)]
    try:
        sol = np.linalg.solve(S + lam * np.diag(np.diag(S)), -g[idx])
    except np.linalg.LinAlgError:
        return d
    if np.isfinite(sol).all():
        d[idx] = sol
    return d


def old_formal_sigma(words, active):
    A, _ = _old_unpack(words, 6)
    out = np.full(6, np.nan)
    out[list(active)] = np.inf
    idx = [j for j in active if A[j, j] > 0]
    p = len(idx)
    if p == 0 or words[2] < p + 1:
        return out
    try:
        cov = np.linalg.inv(A[np.ix_(idx, idx)])
    except np.linalg.LinAlgError:
        return out
    var = (words[3] / (words[2] - p)) * np.diag(cov)
    if np.isfinite(var).all() and (var >= 0).all():
        out[idx] = np.sqrt(var)
    return out


def old_bundle_columns_step(pooled, active, lam):
    A, g = _old_unpack(pooled, 12)
    idx = [c for c in active if A[c, c] > 0]
    d = np.zeros(12)
    if idx:
        S = A[np.ix_(idx, idx)]
        sol = _old_solve_finite(S + lam * np.diag(np.diag(S)), -g[idx])
        if sol is not None:
            d[idx] = sol
    return d


def old_bundle_columns_sigma(pooled, active):
    A, _ = _old_unpack(pooled, 12)
    out = np.full(12, np.nan)
    out[list(active)] = np.inf
    idx = [c for c in active if A[c, c] > 0]
    p = len(idx)
    if p == 0 or pooled[2] < p + 1:
        return out
    cov = _old_solve_finite(A[np.ix_(idx, idx)], np.eye(p))
    if cov is None:
        return out
    var = (pooled[3] / (pooled[2] - p)) * np.diag(cov)
    if np.isfinite(var).all() and (var >= 0).all():
        out[idx] = np.sqrt(var)
    return out


def _words(slots, A, g, inliers=200.0, r2=0.37):
    w = np.zeros(32 if slots == 6 else 96)
    w[0], w[1], w[2], w[3] = inliers + 9, r2 * 1.5, inliers, r2
    w[4:4 + slots] = g
    w[4 + slots:4 + slots + slots * (slots + 1) // 2] = A[np.triu_indices(slots)]
    return w


def _table(slots):
    """(name, words, active): systems of `slots` unknowns with p live unknowns from 0 to all, and the edges of the two rules."""
    rng = np.random.default_rng(100 + slots)
    rows = []
    for p in range(slots + 1):                                      # p of the slots carry a system, the others are exactly zero
        live = sorted(rng.choice(slots, p, replace=False))
        J = np.zeros((60, slots))
        J[:, live] = rng.normal(size=(60, p))
        r = rng.normal(size=60) * 1e-2
        rows.append((f"p={p}", _words(slots, J.T @ J, J.T @ r), list(range(slots))))
        if 0 < p < slots:
            rows.append((f"p={p}, some not active", _words(slots, J.T @ J, J.T @ r), list(range(0, slots, 2))))
    J = rng.normal(size=(60, slots))
    A, g = J.T @ J, J.T @ (rng.normal(size=60) * 1e-2)
    Z = A.copy()
    Z[1, :] = Z[:, 1] = 0.0
    rows.append(("a zero diagonal on an active slot", _words(slots, Z, g), list(range(slots))))
    S = A.copy()
    S[2, :], S[:, 2] = S[0, :], S[:, 0]                              # rows and columns 0 and 2 are the same: singular, diagonal positive
    S[2, 2] = S[0, 0]
    rows.append(("a singular block", _words(slots, S, g), list(range(slots))))
    ones = np.ones((slots, slots))
    rows.append(("a singular block of ones", _words(slots, ones, np.ones(slots)), list(range(slots))))
    rows.append(("fewer inliers than p + 1", _words(slots, A, g, inliers=float(slots)), list(range(slots))))
    rows.append(("exactly p + 1 inliers", _words(slots, A, g, inliers=slots + 1.0), list(range(slots))))
    tiny = np.diag(np.full(slots, 5e-324))
    rows.append(("a solution that is not finite", _words(slots, tiny, np.full(slots, 1e300)), list(range(slots))))
    huge = A * 1e-3
    huge[0, 0] = 1e-320
    rows.append(("a variance that is not finite", _words(slots, np.diag(np.diag(huge)), g, r2=1e300), list(range(slots))))
    return rows


@pytest.mark.parametrize('slots', [6, 12])
def test_public_steps_and_sigmas_return_the_bytes_of_their_former_bodies(slots):
    step, sigma, old_step, old_sigma = ((rf.levenberg_step, rf.formal_sigma, old_levenberg_step, old_formal_sigma) if slots == 6 else
                                        (rf.bundle_columns_step, rf.bundle_columns_sigma, old_bundle_columns_step, old_bundle_columns_sigma))
    seen = set()
    for name, words, active in _table(slots):
        with np.errstate(all='ignore'):
            for lam in (0.0, 1e-3, 10.0):
                got, want = step(words, active, lam), old_step(words, active, lam)
                assert got.shape == (slots,) and got.dtype == np.float64 and got.tobytes() == want.tobytes(), (name, lam, got, want)
            got, want = sigma(words, active), old_sigma(words, active)
            assert got.shape == (slots,) and got.tobytes() == want.tobytes(), (name, got, want)
        if not step(words, active, 0.0).any():
            seen.add('zero step')
        if np.isinf(got).any():
            seen.add('inf sigma')
        if np.isfinite(got[active]).all():
            seen.add('finite sigma')
    assert seen == {'zero step', 'inf sigma', 'finite sigma'}
    # the table's edges are the edges: a singular block and a solution that is not finite give no step, too few inliers no sigma
    rows = {name: (w, a) for name, w, a in _table(slots)}
    with np.errstate(all='ignore'):
        for name in ("a singular block of ones", "a solution that is not finite"):
            assert not step(*rows[name], 0.0).any(), name
        assert np.isinf(sigma(*rows["fewer inliers than p + 1"])).all() and np.isfinite(sigma(*rows["exactly p + 1 inliers"])).all()
        assert sigma(*rows["a zero diagonal on an active slot"])[1] == np.inf and step(*rows["a zero diagonal on an active slot"], 1e-3)[1] == 0
        assert np.isinf(sigma(*rows["a variance that is not finite"])).all()


def test_pools_and_unpacks_keep_their_widths_and_order():
    rng = np.random.default_rng(3)
    for pool, width in ((rf.pool_frames, 32), (rf.pool_bundle, 96)):
        w = rng.normal(size=(7, width)) * 10.0 ** rng.integers(-8, 8, (7, width))
        want = np.zeros(width)
        for row in w:
            want = want + row
        assert pool(w).tobytes() == want.tobytes() and pool(w[:0]).tobytes() == np.zeros(width).tobytes()
    for unpack, slots, width in ((rf.unpack_normal_equations, 6, 32), (rf.unpack_bundle, 12, 96)):
        w = rng.normal(size=width)
        (A, g), (A0, g0) = unpack(w), _old_unpack(w, slots)
        assert A.tobytes() == A0.tobytes() and g.tobytes() == g0.tobytes()


# ---------------------------------------------------------------------------------------------- (b) the shared loop
def test_the_shared_loop_keeps_exactly_the_strict_decreases():
    """Costs 5 (start), then trials 4 (fall), 6 (rise), 4 (equal), 3 (fall), 3 (equal): states are numbered in the order proposed."""
    script = [5.0, 4.0, 6.0, 4.0, 3.0, 3.0]
    evaluated, proposed = [], []

    def evaluate(state):
        evaluated.append(state)
        return ('payload of', state), script[len(evaluated) - 1]

    def propose(state, payload, lam):
        assert payload == ('payload of', state)                    # the payload handed on is the held state's
        proposed.append((state, lam))
        return len(proposed)

    state, payload, first, steps = rf._levenberg_loop(evaluate, propose, 0, 5, 0.5)
    assert evaluated == [0, 1, 2, 3, 4, 5]
    assert proposed == [(0, 0.5), (1, 0.5), (1, 5.0), (1, 50.0), (4, 50.0)]       # refused twice: lam x 10 each time, never divided
    assert (state, payload, first, steps) == (4, ('payload of', 4), ('payload of', 0), 2)
    # no rounds: one evaluation, nothing proposed
    evaluated.clear()
    proposed.clear()
    assert rf._levenberg_loop(evaluate, propose, 'start', 0, 1e-3) == ('start', ('payload of', 'start'), ('payload of', 'start'), 0)
    assert evaluated == ['start'] and proposed == []
    # a cost of inf or nan is never a decrease, and nothing is a decrease from nan
    for costs in ([1.0, np.inf, np.nan], [np.nan, 0.0, -1.0], [np.inf, np.inf, 7.0]):
        it = iter(costs)
        state, _, _, steps = rf._levenberg_loop(lambda s: (s, next(it)), lambda s, p, lam: s + 1, 0, 2, 1.0)
        assert (state, steps) == ((1, 1) if costs[0] == np.inf else (0, 0)), costs


# ---------------------------------------------------------------------------------------------- (c) depth alone
@pytest.mark.parametrize('mode', ['frame', 'offset'])
def test_depth_alone_solves_on_the_words_as_the_kernel_wrote_them(on_the_host, monkeypatch, mode):
    e = StubEngine()
    made, seen = [], []
    real_equations = e.bundle_normal_equations
    monkeypatch.setattr(e, 'bundle_normal_equations', lambda *a: made.append(real_equations(*a)) or made[-1])
    name = 'schur_step' if mode == 'frame' else 'bundle_columns_step'
    real_step = getattr(rf, name)
    monkeypatch.setattr(rf, name, lambda words, *a: seen.append(np.array(words)) or real_step(words, *a))
    res = rf.BundleRefiner(e, _intr(), joints=mode, iterations=3, silhouette=0.0).refine(POSE, ANGLES, DEPTH)
    assert res.steps_taken == 3 and len(made) == 4 and len(seen) == 3
    for k, words in enumerate(seen):                                # every step accepted: round k solves on evaluation k
        want = made[k] if mode == 'frame' else rf.pool_bundle(made[k])
        assert words.shape == want.shape and words.tobytes() == want.tobytes(), k
        assert words[..., 0].all() and words[..., 2].all()         # the counts are there: not the weighted system, whose [0 .. 3] are 0
    assert 'silhouette' not in e.calls and not any(isinstance(c, tuple) for c in e.calls)
