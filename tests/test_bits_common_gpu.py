"""The kernels of csrc/bits_common.hip -- the popcount of every bit row, the int32 sum with and without its positive count, the
row-wise confusion counts -- through the four entry points that between them reach each kernel in each argument form:

    bmf_bits_confusion                      confusion kernel, two sums without a positive count
    bmf_mebf_scores                         row popcounts, one sum with the positive count
    bmf_concept_apply with u = v = NULL     the model's own count kernel, then the shared sum
    bmf_bits_rebuild with f = 0 and a sum   likewise

Rows cross the four rows of a block and the 256 threads of the sum, row lengths the 64 lanes of a wave.  Integers only: every
comparison is equality against NumPy popcounts.  Outputs are pre-filled with a marker and have slots behind them that must keep it;
every tensor that was uploaded stays referenced until the device has been waited for.
"""
import ctypes as C

import numpy as np
import pytest

import bits_ref as R

pytestmark = pytest.mark.gpu

MARK = -7
ROWS = (1, 3, 4, 5, 255, 256, 257)
WORDS = (1, 63, 64, 65, 130)


def matrix(rows, words, kind, seed=0):
    if kind == "random":
        bits = np.random.RandomState(3100 + 131 * rows + words + seed).rand(rows, words * 32) < 0.3
        return np.packbits(bits, axis=1, bitorder="little").view(np.uint32).copy()
    return np.full((rows, words), R.ONES if kind == "ones" else 0, dtype=np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def marked(n, dtype):
    import torch
    return torch.full((n,), MARK, dtype=dtype, device="cuda:0")


def vp(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def check_confusion(P, G):
    import torch
    from pybmf_amd._lib import check, lib
    rows, ld = P.shape
    Pd, Gd, work, counts = dev(P), dev(G), marked(2 * rows + 3, torch.int32), marked(3, torch.int64)
    check(lib.bmf_bits_confusion(vp(Pd), vp(Gd), rows, ld, vp(work), vp(counts), None), "bmf_bits_confusion")
    torch.cuda.synchronize()
    work, counts = work.cpu().numpy(), counts.cpu().numpy()
    tp, n_p = R.popcount_rows(P & G), R.popcount_rows(P)
    assert work[:rows].tolist() == tp.tolist() and work[rows:2 * rows].tolist() == n_p.tolist() and (work[2 * rows:] == MARK).all()
    assert counts.tolist() == [int(tp.sum()), int(n_p.sum()), MARK]
    assert Pd.cpu().numpy().tobytes() == P.tobytes() and Gd.cpu().numpy().tobytes() == G.tobytes()


def check_scores(M):
    import torch
    from pybmf_amd._lib import check, lib
    rows, ld = M.shape
    Md, score, out = dev(M), marked(rows + 3, torch.int32), marked(3, torch.int64)
    check(lib.bmf_mebf_scores(vp(Md), rows, ld, vp(score), vp(out), None), "bmf_mebf_scores")
    torch.cuda.synchronize()
    score, out = score.cpu().numpy(), out.cpu().numpy()
    want = R.popcount_rows(M)
    assert score[:rows].tolist() == want.tolist() and (score[rows:] == MARK).all()
    assert out.tolist() == [int(want.sum()), int((want > 0).sum()), MARK]


def check_apply_counts(RS, PD):
    """u = v = NULL: nothing is applied, the residual is counted row by row and summed."""
    import torch
    from pybmf_amd._lib import check, lib
    rows, ld = RS.shape
    Rd, Pd, count, rsum = dev(RS), dev(PD), marked(rows + 3, torch.int32), marked(2, torch.int64)
    check(lib.bmf_concept_apply(vp(Rd), vp(Pd), rows, ld, None, None, vp(count), vp(rsum), None), "bmf_concept_apply")
    torch.cuda.synchronize()
    count, rsum = count.cpu().numpy(), rsum.cpu().numpy()
    want = R.popcount_rows(RS)
    assert count[:rows].tolist() == want.tolist() and (count[rows:] == MARK).all() and rsum.tolist() == [int(want.sum()), MARK]
    assert Rd.cpu().numpy().tobytes() == RS.tobytes() and Pd.cpu().numpy().tobytes() == PD.tobytes()


def check_rebuild_counts(X):
    """f = 0: an empty prediction, the residual is X, counted row by row and summed."""
    import torch
    from pybmf_amd._lib import check, lib
    rows, ld = X.shape
    Xd, pd, rs = dev(X), marked(rows * ld + 3, torch.int32), marked(rows * ld + 3, torch.int32)
    count, total = marked(rows + 3, torch.int32), marked(2, torch.int64)
    check(lib.bmf_bits_rebuild(vp(Xd), rows, ld, None, None, 1, 0, vp(pd), vp(rs), vp(count), vp(total), None), "bmf_bits_rebuild")
    torch.cuda.synchronize()
    pd, rs, count, total = (t.cpu().numpy() for t in (pd, rs, count, total))
    want = R.popcount_rows(X)
    assert not pd[:rows * ld].any() and rs[:rows * ld].tobytes() == X.tobytes() and (pd[rows * ld:] == MARK).all() and (rs[rows * ld:] == MARK).all()
    assert count[:rows].tolist() == want.tolist() and (count[rows:] == MARK).all() and total.tolist() == [int(want.sum()), MARK]
    assert Xd.cpu().numpy().tobytes() == X.tobytes()


def check_all(P, G):
    check_confusion(P, G)
    empty = P.copy()
    empty[P.shape[0] // 2] = 0            # an empty row: it counts into the sum with 0 and not into the positive counts
    for M in (P, empty):
        check_scores(M)
    check_apply_counts(P, G)
    check_rebuild_counts(P)


@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("rows", ROWS)
def test_random_bits(rows, words):
    check_all(matrix(rows, words, "random"), matrix(rows, words, "random", seed=1))


@pytest.mark.parametrize("kind", ["zeros", "ones"])
def test_all_zero_and_all_ones(kind):
    M, G = matrix(257, 65, kind), matrix(257, 65, "random")
    check_all(M, G)
    check_confusion(G, M)
