"""NumPy restatement of csrc/hyper.hip and of the miner it serves, on packed uint32 words in the engine's layout (bit rows over the m
rows of X, ld = m_pad / 32 words, zero padded).  Plain helpers, no tests: tests/test_hyper_cpu.py and tests/test_hyper_gpu.py import
this module.

    level_step(tid_prev, x_t, pairs)        what bmf_hyper_level writes: (tid_out, cnt)
    evaluate(tid, rs_t, padded, ids)        what bmf_hyper_eval writes for `ids`: (T rows, nT, s)
    mine(X, min_support)                    the stand-in miner: every frequent itemset of length >= 2 with its integer count

The miner's definition (the issue's; believed to be mlxtend's apriori, never checked against it): levels ascend; inside a level the
itemsets are in lexicographic order of their ascending column tuples; an itemset is frequent iff count / m >= min_support in fp64.
mine() works on the dense matrix and joins nothing: it extends every frequent itemset by every larger column, so it shares no code
path with the engine's vertical miner beyond the definition.
"""
import numpy as np

POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def words_of(m):
    """ld of the engine's transposed bit matrices: m_pad / 32 with m_pad a multiple of 512."""
    return -(-max(m, 1) // 512) * 16


def pack_rows(B, words):
    B = np.asarray(B).astype(bool)
    out = np.zeros((B.shape[0], words * 32), dtype=np.uint8)
    out[:, : B.shape[1]] = B
    return np.packbits(out, axis=1, bitorder="little").view(np.uint32).copy()


def unpack_rows(words, length):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    return np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")[:, :length].astype(bool)


def row_popcounts(M):
    M = np.ascontiguousarray(M, dtype=np.uint32)
    return POP8[M.view(np.uint8)].reshape(M.shape[0], -1).sum(axis=1)


def popcount(words):
    return int(POP8[np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8)].sum())


def level_step(tid_prev, x_t, pairs):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = tid_prev[pairs[:, 0]] & x_t[pairs[:, 1]]
    return out, row_popcounts(out).astype(np.int32)


def pad_items(items):
    """The itemsets as one int array (candidates, longest length), padded with -1: the layout bmf_hyper_eval reads."""
    out = np.full((len(items), max(len(I) for I in items)), -1, dtype=np.int32)
    for i, I in enumerate(items):
        out[i, :len(I)] = I
    return out


def evaluate(tid, rs_t, padded, ids):
    """padded: pad_items of every candidate; ids: the candidates to evaluate.  (T rows, nT, s), one entry per id, in the order of ids."""
    ids = np.asarray(ids, dtype=np.int64)
    rs = np.vstack([rs_t, np.zeros((1, rs_t.shape[1]), dtype=rs_t.dtype)])          # the padding columns read this empty row
    rows = rs[np.where(padded[ids] < 0, rs_t.shape[0], padded[ids])]                   # (ids, longest length, words)
    t = tid[ids]
    T = t & np.bitwise_or.reduce(rows, axis=1)
    return T, row_popcounts(T), row_popcounts((rows & t[:, None, :]).reshape(len(ids), -1))


def mine(X, min_support):
    """([itemset, ...], [count, ...]) of the frequent itemsets of length >= 2 of the 0 / 1 matrix X, in the defined order."""
    X = np.asarray(X) != 0
    m, n = X.shape

    def frequent(rows):
        return np.float64(int(rows.sum())) / m >= min_support
    level = [((j,), X[:, j]) for j in range(n) if frequent(X[:, j])]
    sets, counts = [], []
    while level:
        nxt = []
        for cols, rows in level:
            for j in range(cols[-1] + 1, n):
                both = rows & X[:, j]
                if frequent(both):
                    nxt.append((cols + (j,), both))
        nxt.sort(key=lambda e: e[0])
        sets += [list(c) for c, _ in nxt]
        counts += [int(r.sum()) for _, r in nxt]
        level = nxt
    return sets, counts
