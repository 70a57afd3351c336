"""NumPy restatement of csrc/hyperplus.hip on packed uint32 words in the engine's layout (x_t, pd_t: n bit rows over the m rows of X,
ld = m_pad / 32 words; u_t: the factors' T as bit rows of ld words; v: their I as bit rows of n_pad / 32 words; zero padded).  Plain
helpers, no tests: tests/test_hyperplus_cpu.py and tests/test_hyperplus_gpu.py import this module.

    pair_records(u_t, v, x_t, pd_t, n, pairs)     what bmf_hyperplus_pairs writes: a (count, 5) int64 array
    union(u_t, v, a, b, dst)                      what bmf_hyperplus_union leaves: (u_t, v), new arrays
    dense_new_fp(X, P, T, I)                      the definition on dense matrices: zero cells of X in T x I that P does not cover
"""
import numpy as np

from hyper_ref import popcount, unpack_rows


def pair_records(u_t, v, x_t, pd_t, n, pairs):
    k = u_t.shape[0]
    out = np.full((len(pairs), 5), -1, dtype=np.int64)
    for c, (a, b) in enumerate(np.asarray(pairs, dtype=np.int64).reshape(-1, 2)):
        if not (0 <= a < k and 0 <= b < k) or a == b:
            continue
        T, I = u_t[a] | u_t[b], v[a] | v[b]
        cols = np.nonzero(unpack_rows(I[None, :], n)[0])[0]
        out[c] = (popcount(T[None, :] & ~x_t[cols] & ~pd_t[cols]), popcount(T), popcount(I), popcount(u_t[a] & u_t[b]), popcount(v[a] & v[b]))
    return out


def union(u_t, v, a, b, dst):
    u_t, v = u_t.copy(), v.copy()
    u_t[dst], v[dst] = u_t[a] | u_t[b], v[a] | v[b]
    return u_t, v


def dense_new_fp(X, P, T, I):
    X, P = np.asarray(X) != 0, np.asarray(P) != 0
    return int((~X & ~P)[np.ix_(np.asarray(T, dtype=int), np.asarray(I, dtype=int))].sum())
