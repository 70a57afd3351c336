"""GreConD without a GPU: the model's host loop (models/GreConD.py) on a NumPy stand-in that offers the calls of
pybmf_amd.grecond.ConceptEngine (concept / apply / counts / residual_sum / factor_arrays / prediction), against what the reference
produced (tests/golden/g23_grecond.*, written by tests/golden/make_golden_grecond.py).

The stand-in works on packed uint32 words in the engine's layout (one bit row of m_pad / 32 words per column of X) and runs the
batched restatement of get_concept: evaluate a block of the sweep's remaining candidates against the current best_u, take the FIRST
in column order whose score exceeds best_score, continue behind it.  It is first held to the recorded get_concept calls; the real
class on it must then reproduce every case: the same rows with k, score and shape equal as integers, the metric columns equal to the
recorded floats to 1e-12 (ratios of equal integers: the slack is for the order of two divisions), the final U, V cell for cell, the
counts -- including the factor that a tolerance stop truncates (cases b, c).

Case e (an all-zero X) has no reference result: the reference's "No pattern found" stop raises a TypeError inside its own
early_stop (the fixture records that).  What is asserted there is what the stop is meant to do: zero factors, no log row.
"""
import contextlib
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest
from scipy.sparse import csr_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIT_KW = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def popcount(words) -> int:
    return int(POP8[np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8)].sum())


def pack_rows(B, words):
    """Rows of a 0 / 1 matrix as `words` uint32 words each, bit i of word i // 32, zero padded."""
    B = np.asarray(B).astype(bool)
    out = np.zeros((B.shape[0], words * 32), dtype=np.uint8)
    out[:, : B.shape[1]] = B
    return np.packbits(out, axis=1, bitorder="little").view(np.uint32).copy()


def unpack(words, length):
    return np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8), bitorder="little")[:length].astype(bool)


def scan_block(Xt, rs_t, n, best_u, cands, best_score):
    """What bmf_concept_scan returns: (score, |u_j|, |v_j|) per candidate and the position of the first candidate whose score
    exceeds best_score (-1: none).  Packed words throughout; a column is dropped when it fails on the first 8 non-empty words of
    u_j, the others go through the whole test."""
    Xn = Xt[:n]
    not_X = ~Xn
    score, nu, nv = (np.zeros(len(cands), dtype=np.int64) for _ in range(3))
    first = -1
    for i, j in enumerate(cands):
        u = Xt[j] & best_u
        head = np.nonzero(u)[0][:8]
        if head.size == 0:          # the empty set lies in every column and covers nothing
            nv[i] = n
            continue
        alive = np.nonzero(~(u[head] & not_X[:, head]).any(axis=1))[0]
        inside = alive[~(u & not_X[alive]).any(axis=1)]
        nu[i], nv[i], score[i] = popcount(u), inside.size, popcount(u & rs_t[inside])
        if first < 0 and score[i] > best_score:
            first = i
    return score, nu, nv, first


def close_concept(Xt, n, best_u, j, v_words):
    """What bmf_concept_close leaves: (best_u & Xt[j], bit vector over the columns that contain it)."""
    u = Xt[j] & best_u
    inside = ~(u & ~Xt[:n]).any(axis=1)
    return u, pack_rows(inside[None, :], v_words)[0]


class NumpyConceptEngine:
    """pybmf_amd.grecond.ConceptEngine in NumPy, same layout (m_pad, n_pad multiples of 512), same interface."""

    def __init__(self, X, extra=None):
        X = np.asarray(X) != 0
        self.m, self.n = X.shape
        self.W, self.nvw = -(-max(self.m, 1) // 512) * 16, -(-self.n // 512) * 16
        self.Xt = pack_rows(X.T, self.W)
        self.rs_t, self.pd_t = self.Xt.copy(), np.zeros_like(self.Xt)
        self.truth = {"train": self.Xt}
        for name, G in (extra or {}).items():
            self.truth[name] = pack_rows((np.asarray(G) != 0).T, self.W)
        self.all_rows = pack_rows(np.ones((1, self.m)), self.W)[0]
        self._factors = []
        self.launches = self.accepted = 0

    def concept(self, block=None):
        self.launches = self.accepted = 0
        best_score, best_u, best_v = 0, self.all_rows.copy(), np.zeros(self.nvw, dtype=np.uint32)
        col = np.array([popcount(r) for r in self.rs_t[: self.n]], dtype=np.int64)
        j_rs = np.nonzero(col > 0)[0]
        while True:
            last = best_score
            j_list = j_rs[~unpack(best_v, self.nvw * 32)[j_rs]] if j_rs.size else j_rs
            pos = 0
            while pos < len(j_list):
                count = len(j_list) - pos if not block else min(int(block), len(j_list) - pos)
                score, _, _, first = scan_block(self.Xt, self.rs_t, self.n, best_u, j_list[pos:pos + count], best_score)
                self.launches += 1
                if first >= 0:
                    best_score = int(score[first])
                    best_u, best_v = close_concept(self.Xt, self.n, best_u, j_list[pos + first], self.nvw)
                    pos += first + 1
                    self.accepted += 1
                else:
                    pos += count
            if best_score == last:
                break
        return best_score, best_u, best_v

    def apply(self, u, v):
        cols = np.nonzero(unpack(v, self.n))[0]
        self.rs_t[cols] &= ~np.asarray(u, dtype=np.uint32)
        self.pd_t[cols] |= np.asarray(u, dtype=np.uint32)
        self._factors.append((np.array(u, dtype=np.uint32), np.array(v, dtype=np.uint32)))

    def residual_sum(self):
        return popcount(self.rs_t)

    def counts(self, name="train"):
        G = self.truth[name]
        tp, n_pd, n_gt = popcount(self.pd_t & G), popcount(self.pd_t), popcount(G)
        return tp, n_pd - tp, n_gt - tp, self.m * self.n - n_pd - (n_gt - tp)

    def factor_arrays(self):
        U = np.array([unpack(u, self.m) for u, _ in self._factors], dtype=np.uint8).reshape(len(self._factors), self.m).T
        V = np.array([unpack(v, self.n) for _, v in self._factors], dtype=np.uint8).reshape(len(self._factors), self.n).T
        return U, V

    def prediction(self):
        rows = np.unpackbits(self.pd_t[: self.n].view(np.uint8), axis=1, bitorder="little")[:, : self.m]
        return csr_matrix(rows.T.astype(int))


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def load_case(name):
    meta = json.load(open(os.path.join(GOLDEN, "g23_grecond.json")))
    z = np.load(os.path.join(GOLDEN, "g23_grecond.npz"))
    c = dict(meta["cases"][name])
    for key in ("X", "U", "V", "X_val", "X_test"):
        if f"{name}_{key}" in z.files:
            c[key] = z[f"{name}_{key}"]
    for i, p in enumerate(c["points"]):
        for key in ("X_rs", "u", "v"):
            p[key] = z[f"{name}_p{i}_{key}"]
    return c


def numpy_engine(model):
    extra = {name: np.asarray(X.todense()) for name, X in (("val", model.X_val), ("test", model.X_test)) if X is not None}
    return NumpyConceptEngine(np.asarray(model.X_train.todense()), extra)


def fit_case(case, engine_factory=None, block=None):
    """The real class on case's matrices; engine_factory(model) replaces the device engine."""
    from pybmf_amd.models import GreConD

    class Model(GreConD):
        if engine_factory is not None:
            def _make_engine(self):
                return engine_factory(self)

    def sp(key):
        return None if case.get(key) is None else csr_matrix(case[key].astype(np.float64))
    with contextlib.redirect_stdout(io.StringIO()):
        model = Model(k=case["k"], tol=case["tol"])
        model.fit(sp("X"), sp("X_val"), sp("X_test"), **dict(FIT_KW, block=block))
    return model


def log_rows(model):
    """[[k, score, |u|, |v|, metrics ...]] of logs['updates'] (time stamp dropped, the shape cell flattened)."""
    if "updates" not in model.logs:
        return []
    out = []
    for r in model.logs["updates"].values.tolist():
        out.append([r[1], r[2], r[3][0], r[3][1]] + [float(x) for x in r[4:]])
    return out


def check_fit(model, case):
    got, want = log_rows(model), case["log"]["rows"]
    assert len(got) == len(want)
    if case.get("raised"):          # case e: the reference stops with an exception; the stop itself leaves zero factors
        assert model.U.shape == (case["shape"][0], 0) and model.V.shape == (case["shape"][1], 0)
        assert model._engine.counts("train") == (0, 0, int(case["X"].sum()), case["X"].size - int(case["X"].sum()))
        assert model.X_pd.nnz == 0
        return
    n_head = 4
    assert case["log"]["columns"][:n_head] == ["k", "score", "n_u", "n_v"]
    for g, w in zip(got, want):
        assert all(isinstance(x, (int, np.integer)) for x in g[:n_head]), g[:n_head]
        assert [int(x) for x in g[:n_head]] == w[:n_head]
    G, Wt = np.array([r[n_head:] for r in got]), np.array([r[n_head:] for r in want])
    assert G.shape == Wt.shape and np.abs(G - Wt).max() <= 1e-12
    U, V = np.asarray(model.U.todense()), np.asarray(model.V.todense())
    assert U.shape == case["U"].shape and V.shape == case["V"].shape
    assert (U != 0).tolist() == (case["U"] != 0).tolist() and (V != 0).tolist() == (case["V"] != 0).tolist()
    assert list(model._engine.counts("train")) == case["counts"]
    X_pd, X = np.asarray(model.X_pd.todense()), case["X"]
    assert [int((X_pd & X).sum()), int((X_pd & (1 - X)).sum())] == case["counts"][:2]
    assert model._engine.residual_sum() == case["counts"][2]
    # every applied factor is in the engine, the truncated one included
    Ue, Ve = model._engine.factor_arrays()
    assert Ue.shape[1] == len(want) and (Ue[:, : U.shape[1]] != 0).tolist() == (U != 0).tolist() and (Ve[:, : V.shape[1]] != 0).tolist() == (V != 0).tolist()


# ---- tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "e"])
@pytest.mark.parametrize("block", [None, 1, 7])
def test_stand_in_matches_get_concept_at_the_recorded_calls(name, block):
    case = load_case(name)
    assert len(case["points"]) >= 1
    for p in case["points"]:
        eng = NumpyConceptEngine(case["X"])
        eng.rs_t = pack_rows(p["X_rs"].T, eng.W)
        score, u, v = eng.concept(block=block)
        assert score == p["score"]
        assert unpack(u, eng.m).tolist() == (p["u"] != 0).tolist() and unpack(v, eng.n).tolist() == (p["v"] != 0).tolist()
        assert popcount(u) == int(p["u"].sum()) and popcount(v) == int(p["v"].sum())   # padding bits stay zero
        assert eng.launches >= eng.accepted + (1 if score else 0)


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_host_loop_reproduces_the_reference(name):
    case = load_case(name)
    model = fit_case(case, numpy_engine)
    check_fit(model, case)
    rows = case["log"]["rows"]
    if name == "a":      # "Reach requested factor" keeps all k factors
        assert len(rows) == case["k"] == model.U.shape[1]
    if name in ("b", "c"):   # error <= tol: the factor added last is dropped from U, V but not from X_pd or the log
        assert model.U.shape[1] == len(rows) - 1
    if name == "b":
        assert len(rows) > 128
    if name == "c":
        assert model._engine.residual_sum() == 0
    if name == "d":
        assert [c.split("/")[0] for c in case["log"]["columns"][4:]] == ["train"] * 4 + ["val"] * 4 + ["test"] * 4
        assert len(rows[0]) == 16


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_block_size_does_not_change_the_result(name):
    case = load_case(name)
    ref = fit_case(case, numpy_engine)
    for block in (1, 7):
        model = fit_case(case, numpy_engine, block=block)
        assert [r[:4] for r in log_rows(model)] == [r[:4] for r in log_rows(ref)]
        assert (model.U != ref.U).nnz == 0 and (model.V != ref.V).nnz == 0
        check_fit(model, case)


def test_block_size_on_the_long_case():
    """Case b concept by concept (the whole fit three times over would take minutes on the host): the recorded calls at block 1 and 7
    are in test_stand_in_matches_get_concept_at_the_recorded_calls; here the first 12 concepts of the fit."""
    case = load_case("b")
    engines = [NumpyConceptEngine(case["X"]) for _ in range(3)]
    for _ in range(12):
        out = [e.concept(block=b) for e, b in zip(engines, (None, 1, 7))]
        assert out[0][0] == out[1][0] == out[2][0] > 0
        assert out[0][1].tobytes() == out[1][1].tobytes() == out[2][1].tobytes()
        assert out[0][2].tobytes() == out[1][2].tobytes() == out[2][2].tobytes()
        for e in engines:
            e.apply(out[0][1], out[0][2])


def test_refusals():
    from pybmf_amd.models import GreConD
    case = load_case("a")
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(NotImplementedError, match="reconstruction"):
            GreConD(k=2).fit(csr_matrix(case["X"].astype(np.float64)), **dict(FIT_KW, task="prediction"))
        with pytest.raises(NotImplementedError, match="Boolean"):
            GreConD(k=2).fit(case["X"].astype(np.float64) * 3, **FIT_KW)


def test_pack_helpers_agree_with_the_engine_module():
    from pybmf_amd.bitset import pack_bits, unpack_bits
    rng = np.random.RandomState(5)
    for length in (1, 31, 32, 33, 700):
        f = rng.rand(length) < 0.4
        w = pack_bits(f, 32)
        assert w.tobytes() == pack_rows(f[None, :], 32)[0].tobytes()
        assert unpack_bits(w, length).tolist() == f.tolist() and popcount(w) == int(f.sum())


# ---- ABI --------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = {
    "bmf_concept_scan_work": 1, "bmf_concept_scan": 14, "bmf_concept_close": 8, "bmf_concept_apply": 9, "bmf_bits_confusion": 7,
}


def test_entry_points_are_declared_exported_and_bound():
    from pybmf_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmf_hip.h")).read(), flags=re.S)
    raw = C.CDLL(L.LIB_PATH)
    for name, n_args in NEW_ENTRY_POINTS.items():
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, f"{name} is not declared in bmf_hip.h"
        assert len(decl.group(1).split(",")) == n_args
        assert hasattr(raw, name), f"{name} is missing from libbmf_hip.so"
        res, args = L.SIGNATURES[name]
        assert len(args) == n_args and res is (L._i64 if name.endswith("_work") else C.c_int)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from pybmf_amd import _lib as L
    lib = L.lib
    assert lib.bmf_concept_scan_work(0) == -1 and lib.bmf_concept_scan_work(10) == 64 * 10 * 12
    assert lib.bmf_concept_scan(None, None, 4, 16, None, None, 1, 0, None, None, None, None, None, None) == -1
    assert b"null pointer" in lib.bmf_last_error()
    buf = (C.c_int64 * 4096)()
    p = C.cast(buf, C.c_void_p)
    assert lib.bmf_concept_scan(p, p, 4, 1040, p, p, 1, 0, p, p, p, p, p, None) == -1 and b"32256" in lib.bmf_last_error()
    assert lib.bmf_concept_scan(p, p, 4, 16, p, p, 0, 0, p, p, p, p, p, None) == -1
    assert lib.bmf_concept_close(p, 4, 16, 4, None, p, p, None) == -1          # j >= n
    assert lib.bmf_concept_close(p, 4, 16, -1, None, p, p, None) == -1         # j < 0 needs rec
    assert lib.bmf_concept_apply(p, p, 4, 16, p, None, p, p, None) == -1       # u without v
    assert lib.bmf_bits_confusion(p, None, 4, 16, p, p, None) == -1
