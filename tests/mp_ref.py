"""NumPy fp64 restatement of the MessagePassing model of this build (csrc/mp.hip): the max-sum updates of Ravanbakhsh, Poczos
and Greiner (ICML 2016, Algorithm 1) over dense (m, n, k) arrays, the counter-based start, the fit loop, a stand-in engine with the
interface of pybmf_amd.mp.MessagePassingEngine, and the fixtures of the tests.

min / max are the selections a < b ? a : b and a > b ? a : b (the second operand on equality), T is summed by an explicit loop over f,
the damped combination is two products and a sum.  The order of the row / column sums is selectable: 'forward' (ascending index) or
'reversed'."""
import numpy as np

MASK64 = (1 << 64) - 1
U64 = np.uint64


def mn(a, b):
    return np.where(a < b, a, b)


def mx(a, b):
    return np.where(a > b, a, b)


def splitmix64(x):
    """splitmix64 of a uint64 array (wrap-around arithmetic)."""
    with np.errstate(over="ignore"):
        z = x + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def constants(prior_u, prior_v, channel_pos, channel_neg):
    """(cx, cy, co1, co0)"""
    return (float(np.log(prior_u / (1 - prior_u))), float(np.log(prior_v / (1 - prior_v))),
            float(np.log(channel_pos / (1 - channel_neg))), float(np.log((1 - channel_pos) / channel_neg)))


def start_hats(m, n, k, seed, init_scale, pattern=None):
    """(Phi^, Psi^) of shape (m, n, k): init_scale (2 u - 1) on the pattern, u = the top 53 bits of
    splitmix64(splitmix64(seed) + ((which m + i) n + j) k + f), 0 elsewhere."""
    base = splitmix64(np.array([int(seed) & MASK64], dtype=U64))[0]
    with np.errstate(over="ignore"):
        i = np.arange(m, dtype=U64)[:, None, None]
        j = np.arange(n, dtype=U64)[None, :, None]
        f = np.arange(k, dtype=U64)[None, None, :]
        out = []
        for which in (0, 1):
            idx = ((U64(which) * U64(m) + i) * U64(n) + j) * U64(k) + f
            u = (splitmix64(base + idx) >> U64(11)).astype(np.float64) * 2.0 ** -53
            h = init_scale * (2.0 * u - 1.0)
            if pattern is not None:
                h = np.where(np.asarray(pattern, dtype=bool)[:, :, None], h, 0.0)
            out.append(h)
    return out[0], out[1]


def ordered_sum(A, axis, order="forward"):
    """The sum of A along `axis`, term after term in ascending ('forward') or descending ('reversed') index."""
    A = np.moveaxis(A, axis, 0)
    idx = range(A.shape[0]) if order == "forward" else range(A.shape[0] - 1, -1, -1)
    s = np.zeros(A.shape[1:])
    for t in idx:
        s = s + A[t]
    return s


def marginals(PhiH, PsiH, cx, cy, order="forward"):
    """Xi (m, k) = cx + sum_j Phi^, Ups (n, k) = cy + sum_i Psi^ (the prior last)."""
    return ordered_sum(PhiH, 1, order) + cx, ordered_sum(PsiH, 0, order) + cy


def cell_pass(X, pattern, Xi, Ups, PhiH, PsiH, co1, co0, lr):
    """The new hats of every cell of the pattern from the old state (Jacobi); cells outside keep their hats (0)."""
    k = PhiH.shape[2]
    Ph = Xi[:, None, :] - PhiH
    Ps = Ups[None, :, :] - PsiH
    G = mn(mn(Ph + Ps, Ph), Ps)
    pos = mx(G, 0.0)
    T = np.zeros(G.shape[:2])
    for f in range(k):
        T = T + pos[:, :, f]
    if k > 1:
        srt = np.sort(G, axis=2)
        m1, m2 = srt[:, :, -1:], srt[:, :, -2:-1]
        M = np.where(G == m1, m2, m1)
    else:
        M = np.full(G.shape, -np.inf)
    co = np.where(np.asarray(X, dtype=bool), co1, co0)[:, :, None]
    Gh = mn(mx(-M, 0.0), (T[:, :, None] - pos) + co)
    Pn = mx(Gh + Ps, 0.0) - mx(Ps, 0.0)
    Qn = mx(Gh + Ph, 0.0) - mx(Ph, 0.0)
    oml = 1.0 - lr
    A = oml * PhiH + lr * Pn
    B = oml * PsiH + lr * Qn
    if pattern is not None:
        obs = np.asarray(pattern, dtype=bool)[:, :, None]
        A, B = np.where(obs, A, PhiH), np.where(obs, B, PsiH)
    return A, B


class RefEngine:
    """The state and the steps of a fit in NumPy, with the interface of pybmf_amd.mp.MessagePassingEngine."""

    def __init__(self, X, k, pattern=None, prior_u=0.5, prior_v=0.5, channel_pos=0.99, channel_neg=0.99, lr=0.2, init_scale=1e-2,
                 order="forward"):
        self.X = np.asarray(X, dtype=bool)
        self.m, self.n = self.X.shape
        self.k, self.lr, self.init_scale, self.order = int(k), float(lr), float(init_scale), order
        self.pattern = None if pattern is None else np.asarray(pattern, dtype=bool)
        self.cx, self.cy, self.co1, self.co0 = constants(prior_u, prior_v, channel_pos, channel_neg)

    def start(self, seed):
        self.PhiH, self.PsiH = start_hats(self.m, self.n, self.k, seed, self.init_scale, self.pattern)
        self.Xi, self.Ups = marginals(self.PhiH, self.PsiH, self.cx, self.cy, self.order)

    def step(self):
        self.PhiH, self.PsiH = cell_pass(self.X, self.pattern, self.Xi, self.Ups, self.PhiH, self.PsiH, self.co1, self.co0, self.lr)
        Xi, Ups = marginals(self.PhiH, self.PsiH, self.cx, self.cy, self.order)
        d = max(np.abs(Xi - self.Xi).max(), np.abs(Ups - self.Ups).max())
        self.Xi, self.Ups = Xi, Ups
        return float(d)

    def marginals(self):
        return self.Xi.copy(), self.Ups.copy()

    def decisions(self):
        return self.Xi > 0, self.Ups > 0

    def messages(self):
        return self.PhiH.copy(), self.PsiH.copy()


def fit(X, k, pattern=None, tol=1e-4, max_iter=500, seed=0, engine=None, **kw):
    """The loop of the model: stop after the iteration in which d < tol, or after max_iter iterations.
    Returns dict(U, V, Xi, Ups, n_iter, converged, diffs)."""
    eng = RefEngine(X, k, pattern, **kw) if engine is None else engine
    eng.start(seed)
    diffs, converged = [], False
    while len(diffs) < max_iter:
        diffs.append(eng.step())
        if diffs[-1] < tol:
            converged = True
            break
    Xi, Ups = eng.marginals()
    return dict(U=Xi > 0, V=Ups > 0, Xi=Xi, Ups=Ups, n_iter=len(diffs), converged=converged, diffs=diffs)


def boolean_product(U, V):
    return (np.asarray(U, dtype=np.int64) @ np.asarray(V, dtype=np.int64).T) > 0


def confusion(gt, pd, where=None):
    """(TP, FP, FN, TN) of the prediction against the ground truth, over the cells of `where` (all cells when None)."""
    gt, pd = np.asarray(gt, dtype=bool), np.asarray(pd, dtype=bool)
    w = np.ones(gt.shape, dtype=bool) if where is None else np.asarray(where, dtype=bool)
    return (int((gt & pd & w).sum()), int((~gt & pd & w).sum()), int((gt & ~pd & w).sum()), int((~gt & ~pd & w).sum()))


def scores(counts):
    """[Recall, Precision, Accuracy, F1] as pybmf_amd.utils.scores_from_counts gives them."""
    from pybmf_amd.utils import scores_from_counts
    return [float(v) for v in scores_from_counts(*counts)]


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
CONSTS = dict(prior_u=0.4, prior_v=0.4, channel_pos=0.99, channel_neg=0.99, lr=0.2)
TOL, MAX_ITER, SEED = 1e-4, 500, 0

# name: (m, n, k, noise, data seed, masked)
FIXTURES = {
    "a60x50k3_masked": (60, 50, 3, 0.05, 1, True),
    "b33x130k4_full": (33, 130, 4, 0.02, 3, False),
    "b33x130k4_masked": (33, 130, 4, 0.02, 3, True),
    "c97x70k5_masked": (97, 70, 5, 0.05, 2, True),
    "d130x65k2_masked": (130, 65, 2, 0.05, 5, True),
}
NON_CONVERGENT = (97, 70, 5, 0.05, 2, False)


def planted(m, n, k, noise, s):
    """(X noisy, X clean, pattern, U, V): every draw from one RandomState(s), in this order."""
    rs = np.random.RandomState(s)
    U, V = rs.rand(m, k) < 0.3, rs.rand(n, k) < 0.3
    clean = boolean_product(U, V)
    flips = rs.rand(m, n) < noise
    pattern = rs.rand(m, n) < 0.7
    return clean ^ flips, clean, pattern, U, V


_cache = {}


def fixture(name, order="forward"):
    """(X, clean, pattern or None, fit result) of a fixture; fitted once per (name, order) and shared, never modified."""
    key = (name, order)
    if key not in _cache:
        m, n, k, noise, s, masked = FIXTURES[name]
        X, clean, pattern, _, _ = planted(m, n, k, noise, s)
        pat = pattern if masked else None
        _cache[key] = (X, clean, pat, fit(X, k, pat, tol=TOL, max_iter=MAX_ITER, seed=SEED, order=order, **CONSTS))
    return _cache[key]


def check_fixture(res, tol=TOL, max_iter=MAX_ITER):
    """The conditions every parity fixture must meet (on the oracle alone)."""
    assert res["converged"] and res["n_iter"] < max_iter, "the fixture does not converge"
    small = min(np.abs(res["Xi"]).min(), np.abs(res["Ups"]).min())
    assert small >= 0.1, f"a marginal of {small} sits on the decision threshold"
    for d in res["diffs"][-2:]:
        assert abs(d - tol) >= 0.01 * tol, f"d = {d} is within 1 % of tol: n_iter could flip"


def train_csr(X, pattern):
    """X_train as the model takes it: csr of the ones (W = 'full'), or the pattern's cells stored, zeros included (W = 'mask')."""
    from scipy.sparse import csr_matrix
    X = np.asarray(X)
    if pattern is None:
        return csr_matrix(X.astype(np.float64))
    rows, cols = np.nonzero(pattern)
    return csr_matrix((X[rows, cols].astype(np.float64), (rows, cols)), shape=X.shape)


def make_engine(X, k, pattern, lr=0.2):
    """The device engine (pybmf_amd.mp) for X and a pattern given as arrays, with the constants of the fixtures (GPU tests)."""
    from pybmf_amd.engine import BitMatrix
    from pybmf_amd.mp import MessagePassingEngine
    bits = BitMatrix(np.ascontiguousarray(X, dtype=np.uint8), "cuda:0")
    pat = None if pattern is None else BitMatrix(np.ascontiguousarray(pattern, dtype=np.uint8), "cuda:0")
    return MessagePassingEngine(bits, k, pattern=pat, lr=lr, **{key: CONSTS[key] for key in ("prior_u", "prior_v", "channel_pos", "channel_neg")})
