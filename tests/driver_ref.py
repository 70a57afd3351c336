"""NumPy reference of what the multiplicative-update driver (csrc/api.hip) adds on top of the kernels it launches: the log row, the
stopping rule, the gather of the epilogue partials and the slab sums.  Nothing here is imported from the package.

  log_row      the row from the DEFINITION of every column, in fp64 from dense X, U, V -- not from the kernel's expansion
               0.5 (||X||^2 - 2 <X, U V^T> + <U^T U, V^T V>).  tests/test_driver_cpu.py proves it against the oracle and, on dyadic
               inputs, against exact rational arithmetic.
  stop_rule    early_stop() of the reference (models/BaseModelTools.py:326-334) for the three criteria of the MU loop.
  gather_sums  the sums of the epilogue partials in the order gather_body adds them.
  slab_sum_*   the slab sums in the order of each reduction kernel.
"""
import numpy as np

# columns of a log row (include/bmf_hip.h: BMF_LOG_*)
(ITER, ERROR, REC, REG, REGERR, RMSE, MAE, TP, FP, FN, TN, VALID, STOP) = range(13)
LOG_COLS = 16
MODE_PENALTY, MODE_WNMF = 1, 2


def log_row(X, U, V, it, reg, mode=MODE_PENALTY, with_mae=True, thr_u=0.5, thr_v=0.5):
    """Columns ITER .. VALID of log row `it` for the factors U (m x k), V (n x k) on the 0/1 matrix X, as a float64 vector of
    LOG_COLS entries (STOP and the spare columns are left 0).  rec = 0.5 ||X - U V^T||_F^2; reg_err = reg * 0.5 * (sum (U^2 - U)^2 +
    sum (V^2 - V)^2) in PENALTY mode, 0 in WNMF mode; RMSE, MAE over all cells; TP / FP / FN / TN of min(1, (U > thr_u)(V > thr_v)^T)."""
    X = np.asarray(X, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    cells = float(X.shape[0]) * float(X.shape[1])
    R = X - U @ V.T
    sq = float(np.sum(R * R))
    rec = 0.5 * sq
    reg_err = 0.0
    if mode == MODE_PENALTY:
        reg_err = float(reg) * (0.5 * (float(np.sum((U * U - U) ** 2)) + float(np.sum((V * V - V) ** 2))))
    pd = ((U > thr_u).astype(np.int64) @ (V > thr_v).astype(np.int64).T) > 0
    gt = X != 0
    row = np.zeros(LOG_COLS, dtype=np.float64)
    row[ITER] = float(it)
    row[ERROR] = rec + reg_err
    row[REC] = rec
    row[REG] = float(reg)
    row[REGERR] = reg_err
    row[RMSE] = np.sqrt(np.float64(sq) / np.float64(cells))
    row[MAE] = np.float64(np.sum(np.abs(R))) / np.float64(cells) if with_mae else np.nan
    row[TP] = float(np.sum(gt & pd))
    row[FP] = float(np.sum(~gt & pd))
    row[FN] = float(np.sum(gt & ~pd))
    row[TN] = float(np.sum(~gt & ~pd))
    row[VALID] = 1.0
    return row


def watched(row, mode):
    """The value the stopping rule looks at: reg_error for BinaryMFPenalty (BinaryMFPenalty.py:89,112), the error for WNMF."""
    return row[REGERR] if mode == MODE_PENALTY else row[ERROR]


def stop_rule(it, watched_now, previous, tol, min_diff, max_iter):
    """True when iteration `it` is the last one: watched <= tol, |previous - watched| < min_diff, or it > max_iter -- and never at
    iteration 0, whose row is bookkeeping of the initial factors (the reference evaluates the rule inside the loop only)."""
    if it < 1:
        return False
    stop = False
    if watched_now <= tol:
        stop = True
    if it > max_iter:
        stop = True
    if abs(np.float64(previous) - np.float64(watched_now)) < min_diff:
        stop = True
    return stop


def _strided_tree(x):
    """sum of a vector as gather_body adds it: thread t of 256 takes x[t], x[t + 256], ... in turn, starting from 0.0; then the halving
    tree over the 256 partial sums (sh[t] += sh[t + o] for o = 128, 64, ..., 1)"""
    x = np.asarray(x, dtype=np.float64)
    sh = np.zeros(256, dtype=np.float64)
    for b0 in range(0, len(x), 256):
        seg = x[b0:b0 + 256]
        sh[:len(seg)] = sh[:len(seg)] + seg
    o = 128
    while o > 0:
        sh[:o] = sh[:o] + sh[o:2 * o]
        o >>= 1
    return sh[0]


def gather_sums(partU, partV):
    """(comm[0], comm[1], scal[0]) = (sum U o (X V), sum (U^2 - U)^2, sum (V^2 - V)^2) from the epilogue partials partU [nbU][2],
    partV [nbV][2] ([b][0] the regulariser term, [b][1] the dot term of 128-row block b), in the kernel's order."""
    partU = np.asarray(partU, dtype=np.float64).reshape(-1, 2)
    partV = np.asarray(partV, dtype=np.float64).reshape(-1, 2)
    return _strided_tree(partU[:, 1]), _strided_tree(partU[:, 0]), _strided_tree(partV[:, 0])


def slab_sum_seq(slabs):
    """float32(fp64 sum over the slabs in slab order, from 0.0): reduce_slabs_wide_kernel and the reduction blocks of
    reduce_finalize_kernel.  slabs: [count][...] float32."""
    acc = np.zeros(slabs.shape[1:], dtype=np.float64)
    for s in slabs:
        acc = acc + s.astype(np.float64)
    return acc.astype(np.float32)


def slab_sum_grouped(slabs, groups=16):
    """reduce_slabs_kernel: `groups` contiguous ranges of ceil(count / groups) slabs are summed in fp64 each from 0.0, then the range
    sums are added in range order from 0.0.  Up to `groups` slabs this is slab_sum_seq."""
    count = slabs.shape[0]
    per = -(-count // groups)
    tot = np.zeros(slabs.shape[1:], dtype=np.float64)
    for g in range(groups):
        acc = np.zeros(slabs.shape[1:], dtype=np.float64)
        for s in slabs[g * per:min((g + 1) * per, count)]:
            acc = acc + s.astype(np.float64)
        tot = tot + acc
    return tot.astype(np.float32)


def slab_sum_f32(slabs):
    """the fp32 sum over the slabs in slab order, from +0.0: reduce_slabs_block_kernel"""
    acc = np.zeros(slabs.shape[1:], dtype=np.float32)
    for s in slabs:
        acc = (acc + s.astype(np.float32)).astype(np.float32)
    return acc


# ------------------------------------------------------------------------------------------------------------------------------
# hand-made states of bmf_penalty_finalize: dyadic factors, so that every sum the kernel or the definition forms is exact in fp64
# whatever its order and whether or not a product is contracted into an FMA
# ------------------------------------------------------------------------------------------------------------------------------
DYADIC = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 1.25])


def dyadic_case(k, m=40, n=30, seed=0):
    """(X, U, V): a 0/1 X (m x n, uint8) and factors with entries in {0, 1/4, 1/2, 3/4, 1, 5/4}"""
    rs = np.random.RandomState(1000 * k + seed)
    X = (rs.rand(m, n) < 0.3).astype(np.uint8)
    U = DYADIC[rs.randint(0, len(DYADIC), size=(m, k))]
    V = DYADIC[rs.randint(0, len(DYADIC), size=(n, k))]
    return X, U, V


def finalize_inputs(X, U, V, kp, thr_u=0.5, thr_v=0.5):
    """What finalize_kernel reads, derived on the host from dense X, U, V: comm (8 + kp * kp doubles: [0] <X, U V^T>, [1] sum (U^2 - U)^2,
    [2] TP, [3] FP, [4] sum |X - U V^T|, [5] sum (X - U V^T)^2, [8..] U^T U zero padded to kp x kp), GV64 (V^T V, kp x kp) and
    scal0 = sum (V^2 - V)^2."""
    X = np.asarray(X, dtype=np.float64)
    k = U.shape[1]
    P = U @ V.T
    comm = np.zeros(8 + kp * kp, dtype=np.float64)
    comm[0] = np.sum(X * P)
    comm[1] = np.sum((U * U - U) ** 2)
    pd = ((U > thr_u).astype(np.int64) @ (V > thr_v).astype(np.int64).T) > 0
    comm[2] = float(np.sum((X != 0) & pd))
    comm[3] = float(np.sum((X == 0) & pd))
    comm[4] = np.sum(np.abs(X - P))
    comm[5] = np.sum((X - P) ** 2)
    G = np.zeros((kp, kp), dtype=np.float64)
    G[:k, :k] = U.T @ U
    comm[8:] = G.ravel()
    GV = np.zeros((kp, kp), dtype=np.float64)
    GV[:k, :k] = V.T @ V
    return {"comm": comm, "GV64": GV.ravel(), "scal0": float(np.sum((V * V - V) ** 2))}
