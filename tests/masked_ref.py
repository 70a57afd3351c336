"""fp64 restatements of the observed-cell kernels of csrc/masked.hip and csrc/thresh64.hip, cell by cell over a (row, col, x, w) list.
Plain helpers, no tests: tests/test_masked_kernels_cpu.py pins them to the golden-pinned oracle on a dense scatter of the same cells,
tests/test_masked_kernels_gpu.py compares every kernel variant with them.  NumPy only, float64 throughout; the per-cell scalars are
computed for the whole list at once, the sums are accumulated cell after cell in list order."""
import numpy as np

import oracle as orc

LINK_PLAIN, LINK_SIGMOID, LINK_KL = 0, 1, 2      # BMF_LINK_* of include/bmf_hip.h
WEIGHTS = (0.5, 1.0, 3.0)
REAL_VALUES = (0.0, 0.5, 1.0, 2.0, 5.0)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _cell_weights(w, nnz):
    return np.ones(nnz) if w is None else _f64(w)


def segments_ref(rows, cols, x, w, Fself, Fother, link, lamda):
    """(num, den, sums) of bmf_masked_link_pass over the cells e = (rows[e], cols[e]) with value x[e] and weight w[e] (None: 1), by the
    formulas of the header comment of csrc/masked.hip; p_e = <Fself[rows[e]], Fother[cols[e]]>:
      plain    num[r] += w x F_other[j],  den[r] += w p F_other[j],  sums += (w (x - p)^2, w |x - p|)
      sigmoid  s = lamda (p - 1/2), sig = sigmoid(s), d = sig (1 - sig):  num[r] += lamda w x d F_other[j],  den[r] += lamda w sig d F_other[j],
               sums += (w (x - sig)^2, w |x - sig|)        (1 - sig is taken as sigmoid(-s): no cancellation in the upper tail)
      KL       num[r] += w x / p F_other[j] over the cells with x != 0,  den = 0,  sums[0] += 2 w (x log(x / p) - x + p) with
               0 log 0 = 0 and no clamp of p,  sums[1] = 0."""
    rows, cols, x = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), _f64(x)
    Fself, Fother = _f64(Fself), _f64(Fother)
    w = _cell_weights(w, len(rows))
    p = np.einsum("ek,ek->e", Fself[rows], Fother[cols])
    sums = np.zeros(2)
    if link == LINK_PLAIN:
        cn, cd, pred = w * x, w * p, p
    elif link == LINK_SIGMOID:
        s = lamda * (p - 0.5)
        sig = orc.stable_sigmoid(s)
        d = sig * orc.stable_sigmoid(-s)
        cn, cd, pred = lamda * w * x * d, lamda * w * sig * d, sig
    elif link == LINK_KL:
        nz = x != 0
        cn, cd = np.zeros(len(rows)), np.zeros(len(rows))
        cn[nz] = w[nz] * x[nz] / p[nz]
        kl = p - x
        kl[nz] += x[nz] * np.log(x[nz] / p[nz])
    else:
        raise ValueError(link)
    num, den = np.zeros(Fself.shape), np.zeros(Fself.shape)
    for e in range(len(rows)):
        v = Fother[cols[e]]
        num[rows[e]] += cn[e] * v
        den[rows[e]] += cd[e] * v
        if link == LINK_KL:
            sums[0] += 2.0 * w[e] * kl[e]
        else:
            r = x[e] - pred[e]
            sums[0] += w[e] * r * r
            sums[1] += w[e] * abs(r)
    return num, den, sums


def thresh_cells_ref(rows, cols, x, w, Us, dUs, Vs, dVs):
    """(sum (w r)^2, g1, g2) over the cells from TRANSFORMED factors: r = x - <Us[i], Vs[j]>, g1 = sum w r <dUs[i], Vs[j]>,
    g2 = sum w r <Us[i], dVs[j]>: the weight squared in the objective, once in the gradient (BinaryMFThreshold.py:169-170, :195-206)."""
    rows, cols, x = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), _f64(x)
    Us, dUs, Vs, dVs = _f64(Us), _f64(dUs), _f64(Vs), _f64(dVs)
    w = _cell_weights(w, len(rows))
    f = g1 = g2 = 0.0
    for e in range(len(rows)):
        i, j = rows[e], cols[e]
        r = x[e] - float(Us[i] @ Vs[j])
        f += (w[e] * r) ** 2
        g1 += w[e] * r * float(dUs[i] @ Vs[j])
        g2 += w[e] * r * float(Us[i] @ dVs[j])
    return f, g1, g2


def thresh_ref(rows, cols, x, w, U, V, u, v, lamda):
    """The same from the raw factors: Us = sigmoid(lamda (U - u)), dUs = dXdx(U, u), likewise V.  F = half the first value; (g1, g2) is
    the 2-vector the reference calls dF, in its sign convention (oracle.thresh_dF)."""
    U, V = _f64(U), _f64(V)
    return thresh_cells_ref(rows, cols, x, w, orc.stable_sigmoid((U - u) * lamda), orc.thresh_dXdx(U, u, lamda),
                            orc.stable_sigmoid((V - v) * lamda), orc.thresh_dXdx(V, v, lamda))


def counts_ref(rows, cols, x, ubits, vbits):
    """(TP, FP, FN, TN) as Python ints: pd = (ubits[row] & vbits[col]) != 0, gt = x != 0."""
    c = [0, 0, 0, 0]
    for i, j, xv in zip(np.asarray(rows).tolist(), np.asarray(cols).tolist(), np.asarray(x).tolist()):
        pd = (int(ubits[i]) & int(vbits[j])) != 0
        gt = xv != 0
        c[(0 if pd else 2) if gt else (1 if pd else 3)] += 1
    return tuple(c)


def make_cells(row_lengths, n, rs, real=False, weights=False, density=0.4, full_col=None):
    """A cell list in which row i holds exactly row_lengths[i] distinct columns of 0 .. n - 1, row-major with increasing columns.
    Values: Boolean (ones with probability `density`) or, real=True, drawn from REAL_VALUES (stored zeros included); weights=True
    draws them from WEIGHTS, else None.  full_col: a column that every non-empty row holds.  Returns (rows, cols, x, w)."""
    rows, cols = [], []
    for i, ln in enumerate(row_lengths):
        assert 0 <= ln <= n
        if full_col is not None and ln >= 1:
            others = np.delete(np.arange(n), full_col)
            c = np.append(rs.choice(others, size=ln - 1, replace=False), full_col)
        else:
            c = rs.choice(n, size=ln, replace=False)
        cols.append(np.sort(c))
        rows.append(np.full(ln, i, dtype=np.int64))
    rows, cols = np.concatenate(rows), np.concatenate(cols).astype(np.int64)
    nnz = len(rows)
    x = rs.choice(REAL_VALUES, size=nnz) if real else (rs.rand(nnz) < density).astype(np.float64)
    w = rs.choice(WEIGHTS, size=nnz) if weights else None
    return rows, cols, x, w


def scatter(rows, cols, x, w, shape):
    """The cell list as dense (X, W): W = w at the listed cells (1 without weights), 0 elsewhere."""
    X, W = np.zeros(shape), np.zeros(shape)
    X[rows, cols] = x
    W[rows, cols] = 1.0 if w is None else w
    return X, W
