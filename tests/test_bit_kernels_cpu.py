"""tests/bits_ref.py is right, and its case tables discriminate -- without a GPU and without the library.

1. Every packed-word restatement against the dense definitions the project already trusts (oracle.boolean_product,
   oracle.confusion_counts, oracle.confusion_counts_axis) at small ragged shapes.
2. Every case of the shared tables is non-degenerate (TP > 0, FP > 0, an all-zero row word, a row with bit kp - 1), and every case with
   padding would give another answer if the padding were counted.
3. The cover-count table reaches what it claims: the five reachable wide instantiations, a ragged chunk in one and in several chunk
   columns, a second trip of the row loop in both kernels, and both row-group schemes of the narrow kernel -- by the launch arithmetic
   restated in bits_ref.cover_launch_plan, which is itself checked here against figures worked out by hand from csrc/cover.hip."""
import math

import numpy as np
import pytest

import bits_ref as R
import oracle as orc

SHAPES = [(m, n, k) for m in (1, 63, 65) for n in (1, 31, 33, 129) for k in (1, 32, 33, 64)]


def dense_problem(m, n, k, seed=0):
    rs = np.random.RandomState(1000 * m + 10 * n + k + seed)
    X = (rs.rand(m, n) < 0.3).astype(np.int64)
    Ub = (rs.rand(m, k) < 0.1).astype(np.int64)
    Vb = (rs.rand(n, k) < 0.2).astype(np.int64)
    Ub[0, :] = 0
    Ub[0, k - 1] = 1
    Vb[0, k - 1] = 1
    return X, Ub, Vb


def words_of(D):
    """dense 0/1 rows -> uint32 words (NumPy's own packbits, not bits_ref)"""
    D = np.asarray(D, dtype=np.uint8)
    b = np.zeros((D.shape[0], (D.shape[1] + 31) // 32 * 32), np.uint8)
    b[:, :D.shape[1]] = D
    return np.ascontiguousarray(np.packbits(b, axis=1, bitorder="little")).view(np.uint32)


def dense_of(W, n):
    return np.unpackbits(np.ascontiguousarray(W).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(np.int64)


def row_words_of(Ub):
    return (Ub.astype(np.uint64) << np.arange(Ub.shape[1], dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


# ---- 1. the restatements against the dense definitions --------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_packed_reference_matches_the_dense_definitions(m, n, k):
    X, Ub, Vb = dense_problem(m, n, k)
    Xw, u, colw = words_of(X), row_words_of(Ub), words_of(Vb.T)
    words = Xw.shape[1]
    pd = orc.boolean_product(Ub, Vb)
    got = R.product_words(u, colw, words)
    assert np.array_equal(dense_of(got, n), pd)
    assert not dense_of(got, 32 * words)[:, n:].any()
    assert np.array_equal(R.product_words(u.view(np.int64), colw, words), got)       # the int64 view the device tensors hold
    tp, fp, fn, tn = orc.confusion_counts(X, pd)
    assert R.cover_counts(Xw, words, u, colw) == (tp, fp)
    assert R.cover_counts(Xw, words, u, colw, row_block=7) == (tp, fp)
    rtp, rfp = R.confusion_rows(Xw, got, words)
    wtp, wfp, _, _ = orc.confusion_counts_axis(X, pd, axis=1)
    assert np.array_equal(rtp, wtp) and np.array_equal(rfp, wfp)
    ctp, cfp = R.confusion_rows(words_of(X.T), words_of(pd.T), (m + 31) // 32)
    wtp, wfp, _, _ = orc.confusion_counts_axis(X, pd, axis=0)
    assert np.array_equal(ctp, wtp) and np.array_equal(cfp, wfp)
    assert R.popcount(Xw) == int(X.sum()) and np.array_equal(R.popcount_rows(Xw), X.sum(axis=1))


@pytest.mark.parametrize("cols", [1, 31, 32, 33, 63, 64, 65, 129])
def test_pack_rows_matches_packbits(cols):
    rs = np.random.RandomState(cols)
    X = R.PACK_BYTES[rs.randint(0, len(R.PACK_BYTES), size=(6, cols + 7))]
    X[:, cols:] = 255
    got = R.pack_rows(X, cols)
    assert got.dtype == np.uint32 and got.shape == (6, 2 * ((cols + 63) // 64))
    assert np.array_equal(dense_of(got, cols), (X[:, :cols] != 0).astype(np.int64))
    assert not dense_of(got, 32 * got.shape[1])[:, cols:].any()


def test_popcount_table_and_shapes():
    assert R.POP16[0] == 0 and R.POP16[0xFFFF] == 16 and R.POP16[0x8001] == 2
    w = np.array([[0xFFFFFFFF, 0x80000000, 0, 1]], dtype=np.uint32)
    assert R.popcount(w) == 34 and R.popcount(w[0]) == 34 and R.popcount_rows(w).tolist() == [34]
    assert R.popcount(np.zeros((3, 0), np.uint32)) == 0


def test_sqdiff_and_reduce_slabs_match_their_definitions():
    rs = np.random.RandomState(5)
    A, B, W = (rs.randint(-8, 9, size=1000).astype(np.float64) for _ in range(3))
    W = np.abs(W)
    assert R.sqdiff(A, B, W) == float((W * (A - B) ** 2).sum()) and R.sqdiff(A, B) == float(((A - B) ** 2).sum())
    A, B, W = rs.randn(1000), rs.randn(1000), rs.rand(1000)
    assert math.isclose(R.sqdiff(A, B, W), (W * (A - B) ** 2).sum(), rel_tol=1e-13)
    # fsum is what makes it a reference: terms whose plain left-to-right sum loses the small ones
    assert R.sqdiff(np.array([2.0 ** 27, 1.0, 1.0, 1.0, 1.0]), np.zeros(5)) == 2.0 ** 54 + 4.0
    slabs = rs.randint(0, 1 << 20, size=5 * 12).astype(np.float32)
    got = R.reduce_slabs(slabs, 12, 5, 9)
    assert got.dtype == np.float64 and np.array_equal(got, slabs.reshape(5, 12)[:, :9].astype(np.float64).sum(axis=0))
    assert np.array_equal(R.reduce_slabs(slabs, 12, 3, 12), slabs.reshape(5, 12)[:3].astype(np.float64).sum(axis=0))


def test_input_makers():
    rng = np.random.default_rng(1)
    w = R.random_words(rng, (64, 1024))
    assert abs(R.popcount(w) / (32.0 * w.size) - 0.3125) < 0.002       # about 0.3
    for kp in (32, 64):
        u = R.factor_row_words(rng, 4096, kp)
        bits = R.popcount_rows(np.ascontiguousarray(u).view(np.uint32).reshape(-1, 2))
        assert all(((bits == c).sum() > 200) for c in (0, 1, 2)) and (bits > 8).sum() > 200
        assert kp == 64 or not (u >> np.uint64(kp)).any()
        assert u[0] == np.uint64(1) << np.uint64(kp - 1) and u[1] == 0 and bits[2] == kp
        u2 = R.factor_row_words(rng, 4096, kp, max_bits=2)
        assert R.popcount_rows(np.ascontiguousarray(u2).view(np.uint32).reshape(-1, 2)).max() == 2
    p = R.padded(np.zeros((2, 3), np.uint32), 5)
    assert p.shape == (2, 5) and (p[:, 3:] == 0xFFFFFFFF).all() and not p[:, :3].any()


# ---- 2. the tables discriminate ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kp", R.COVER_PARAMS)
def test_cover_cases_are_non_degenerate_and_padding_would_show(name, kp):
    c = R.cover_case(name, kp)
    assert c["rows_pad"] % 64 == 0 and c["words"] % 4 == 0 and c["ldx"] % 4 == 0 and c["ldcb"] % 4 == 0      # the C ABI's promises
    assert c["X"].shape == (c["rows_pad"], c["ldx"]) and c["colw"].shape == (kp, c["ldcb"]) and c["u"].shape == (c["rows_pad"],)
    assert c["tp"] > 0 and c["fp"] > 0
    assert (c["u"] == 0).any() and ((c["u"] >> np.uint64(kp - 1)) & np.uint64(1)).any()
    assert kp == 64 or not (c["u"] >> np.uint64(kp)).any()
    if c["ldx"] > c["words"] or c["ldcb"] > c["words"]:
        assert (c["X"][:, c["words"]:] == 0xFFFFFFFF).all() and (c["colw"][:, c["words"]:] == 0xFFFFFFFF).all()
        wide = min(c["ldx"], c["ldcb"])
        tp2, fp2 = R.cover_counts(c["X"], wide, c["u"], c["colw"])
        assert tp2 > c["tp"] and fp2 == c["fp"]      # ones in both paddings: every covered padding bit would be a true positive
        # X's rows read with the wrong leading dimension (ldx taken for words) give another count too
        Xbad = np.ascontiguousarray(c["X"]).reshape(-1)[:c["rows_pad"] * c["words"]].reshape(c["rows_pad"], c["words"])
        assert R.cover_counts(Xbad, c["words"], c["u"], c["colw"]) != (c["tp"], c["fp"])


def test_other_cases_are_non_degenerate_and_padding_would_show():
    for name, rows, words, dcb, do in R.PRODUCT_CASES:
        for kp in (32, 64):
            c = R.product_case(name, kp)
            assert c["want"].any() and ((c["u"] >> np.uint64(kp - 1)) & np.uint64(1)).any() and (rows == 1 or (c["u"] == 0).any())
            assert rows < 3 or c["u"][2] == np.uint64((1 << kp) - 1)                  # bit 63 at kp = 64
            if dcb:   # colbits rows read with ldcb taken for words
                bad = np.ascontiguousarray(c["colw"]).reshape(-1)[:kp * words].reshape(kp, words)
                assert not np.array_equal(R.product_words(c["u"], bad, words), c["want"])
    assert max(r * w for _, r, w, _, _ in R.PRODUCT_CASES) > 8192 * 256
    for case in R.CONFUSION_CASES:
        c = R.confusion_case(*case)
        assert c["tp"].sum() > 0 and c["fp"].sum() > 0
        if c["ldg"] > c["words"] or c["ldp"] > c["words"]:
            assert c["ldg"] != c["ldp"]
            tp2, fp2 = R.confusion_rows(R.padded(c["G"], c["words"] + 4), R.padded(c["P"], c["words"] + 4), c["words"] + 1)
            assert (tp2 > c["tp"]).all()
    assert max(c[0] for c in R.CONFUSION_CASES) > 4096 * 4 and {c[1] for c in R.CONFUSION_CASES} >= {1, 63, 64, 65, 130}
    for case in R.PACK_CASES:
        c = R.pack_case(*case)
        assert c["want"].any() and set(np.unique(c["X"][:, :c["cols"]]).tolist()) <= {0, 1, 2, 255}
        assert c["rows"] * c["cols"] < 100 or set(np.unique(c["X"][:, :c["cols"]]).tolist()) == {0, 1, 2, 255}
        if c["ldx"] > c["cols"]:
            assert (c["X"][:, c["cols"]:] == 255).all()
            if c["cols"] % 64:      # a kernel without the `col < cols` mask packs the padding bytes into the last pair
                assert not np.array_equal(R.pack_rows(c["X"], min(c["ldx"], 64 * (c["need"] // 2)))[:, :c["need"]], c["want"])
            bad = np.ascontiguousarray(c["X"]).reshape(-1)[:c["rows"] * c["cols"]].reshape(c["rows"], c["cols"])
            assert not np.array_equal(R.pack_rows(bad, c["cols"]), c["want"])         # ldx taken for cols
    assert max(c[0] * ((c[1] + 63) // 64) for c in R.PACK_CASES) > 8192 * 4
    assert max(r * w for r, w, _ in R.POPCOUNT_CASES) > 2048 * 256 == 524288
    assert max(R.SQDIFF_N) > 1024 * 256 and max(R.REDUCE_N) >= 65536


# ---- 3. what the cover table reaches ----------------------------------------------------------------------------------------------
def test_launch_plan_restatement_by_hand():
    """Figures worked out by hand from bmf_cover_launch for 256 compute units."""
    P = R.cover_launch_plan
    for words, pair in [(128, (0, 2)), (256, (1, 0)), (384, (1, 2)), (512, (2, 0)), (640, (2, 2)), (132, (1, 0)), (260, (1, 2)), (388, (2, 0)),
                        (516, (2, 2)), (636, (2, 2))]:
        p = P(192, words)
        assert (p["kernel"], p["n4"], p["tw"], p["cols"]) == ("wide", pair[0], pair[1], 1), words
        assert p["last_chunk"] == words and p["ragged"] == (words % 128 != 0)
        assert (p["groups"], p["rows_per_block"], p["rows_per_wave"]) == (3, 64, 4)
    for words, cw, cols, last, pair in [(644, 384, 2, 260, (1, 2)), (1284, 512, 3, 260, (2, 0)), (1924, 512, 4, 388, (2, 0))]:
        p = P(128, words)
        assert (p["cw"], p["cols"], p["last_chunk"], p["ragged"], (p["n4"], p["tw"])) == (cw, cols, last, True, pair)
    # no reachable chunk size selects a tail of four words per lane: cw is a multiple of 128
    assert {(p["n4"], p["tw"]) for p in (P(64, w) for w in range(128, 4000, 4))} == {(0, 2), (1, 0), (1, 2), (2, 0), (2, 2)}
    p = P(64 * 257, 128)
    assert (p["groups"], p["rows_per_block"], p["last_block_rows"]) == (129, 128, 64)
    p = P(64 * 4097, 128)
    assert (p["groups"], p["rows_per_block"], p["rows_per_wave"], p["last_block_rows"]) == (241, 1088, 68, 1088)
    p = P(64 * 2047, 4)
    assert (p["kernel"], p["scheme"], p["groups"], p["rows_per_block"], p["last_block_rows"]) == ("narrow", "equal", 512, 256, 192)
    p = P(64 * 2048, 4)
    assert (p["scheme"], p["y_big"], p["rows_big"], p["rows_per_block"], p["rows_per_wave"]) == ("two-size", 256, 384, 128, 48)
    assert p["y_big"] * p["rows_big"] + (p["groups"] - p["y_big"]) * p["rows_per_block"] == 64 * 2048
    p = P(64 * 4100, 8)
    assert (p["scheme"], p["y_big"], p["rows_big"], p["rows_per_block"], p["rows_per_wave"]) == ("two-size", 256, 704, 384, 88)
    assert P(64, 124)["kernel"] == "narrow" and P(64, 128)["kernel"] == "wide"


def plans(cus=R.CUS_MI355X):
    return {c[0]: R.cover_launch_plan(R.cover_rows_pad(c[0], cus), c[2], cus) for c in R.COVER_CASES}


def test_cover_table_reaches_every_launch_path():
    pl = plans()
    wide = {n: p for n, p in pl.items() if p["kernel"] == "wide"}
    narrow = {n: p for n, p in pl.items() if p["kernel"] == "narrow"}
    # all five reachable wide instantiations, each with a full and with a ragged chunk
    assert {(p["n4"], p["tw"]) for p in wide.values()} == {(0, 2), (1, 0), (1, 2), (2, 0), (2, 2)}
    assert {(p["n4"], p["tw"]) for p in wide.values() if not p["ragged"]} == {(0, 2), (1, 0), (1, 2), (2, 0), (2, 2)}
    assert {(p["n4"], p["tw"]) for p in wide.values() if p["ragged"] and p["cols"] == 1} == {(1, 0), (1, 2), (2, 0), (2, 2)}
    # a ragged last chunk in one and in several chunk columns
    assert {p["cols"] for p in wide.values() if p["ragged"]} == {1, 2, 3, 4}
    assert {(n, p["cw"], p["last_chunk"]) for n, p in wide.items() if p["cols"] > 1} == {("cols2", 384, 260), ("cols3", 512, 260), ("cols4", 512, 388)}
    # two lanes of the two-word tail segment on: the chunk ends 4 words into the tail
    for n in ("ragged260", "ragged516", "cols2"):
        p = pl[n]
        assert p["tw"] == 2 and p["last_chunk"] - 256 * p["n4"] == 4
    # row groups of the wide kernel: one unit in one block, a short last block, a second trip of the 64-row loop with a tail
    assert (pl["unit"]["groups"], pl["unit"]["rows_per_block"]) == (1, 64)
    assert pl["shortlast"]["groups"] > 1 and 0 < pl["shortlast"]["last_block_rows"] < pl["shortlast"]["rows_per_block"]
    assert 64 < pl["tall_wide"]["rows_per_wave"] < 128
    assert all(p["rows_per_wave"] <= 64 for n, p in wide.items() if n != "tall_wide")
    # the narrow kernel: both row-group schemes, the largest equal-group shape, and a second trip with a short tail on the big groups
    assert {p["scheme"] for p in narrow.values()} == {"equal", "two-size"}
    assert pl["narrow_equal_max"]["scheme"] == "equal" and R.cover_rows_pad("narrow_equal_max") + 64 == R.cover_rows_pad("narrow_two_size")
    assert pl["narrow_two_size"]["scheme"] == "two-size" and pl["narrow_two_size"]["rows_per_wave"] <= 64
    assert pl["narrow_two_size_g2"]["scheme"] == "two-size" and pl["narrow_two_size_g2"]["rows_per_wave"] == 88
    assert {R.COVER_CASES[i][2] for i in range(len(R.COVER_CASES)) if pl[R.COVER_CASES[i][0]]["kernel"] == "narrow"} >= {4, 8, 16, 124}
    # leading dimensions beyond words on both kernels; words that are a multiple of 4 but not of 16; kp = 32 on both kernels
    ld = [c for c in R.COVER_CASES if c[3] or c[4]]
    assert {pl[c[0]]["kernel"] for c in ld} == {"wide", "narrow"} and all(c[3] != c[4] for c in ld)
    assert any(c[2] % 16 for c in R.COVER_CASES if pl[c[0]]["kernel"] == "wide") and any(c[2] % 16 for c in R.COVER_CASES if pl[c[0]]["kernel"] == "narrow")
    assert {pl[n]["kernel"] for n, kp in R.COVER_PARAMS if kp == 32} == {"wide", "narrow"}
    assert ("full128", 32) in R.COVER_PARAMS and ("ragged132", 32) in R.COVER_PARAMS
    assert all((n, 32) in R.COVER_PARAMS for n in narrow if n != "narrow_ld") and all((c[0], 64) in R.COVER_PARAMS for c in R.COVER_CASES)


@pytest.mark.parametrize("cus", [64, 104, 228, 304])
def test_cover_table_keeps_its_paths_on_other_compute_unit_counts(cus):
    """The row counts follow the device's compute units, so the second trip of the wide row loop is reached on any of them."""
    pl = plans(cus)
    assert 64 < pl["tall_wide"]["rows_per_wave"] < 128 and pl["shortlast"]["groups"] > 1
    assert {(p["n4"], p["tw"]) for p in pl.values() if p["kernel"] == "wide"} == {(0, 2), (1, 0), (1, 2), (2, 0), (2, 2)}
