"""GreConD+ without a GPU: the NumPy stand-in (tests/grecondplus_ref.py) against what the reference produced
(tests/golden/g29_grecondplus.*, written by tests/golden/make_golden_grecondplus.py), and the model's host loop
(models/GreConDPlus.py) on that stand-in.

Everything is integers or bit-identical fp64, so every comparison is exact -- factors, extensions, the step sequence of every
expansion with both scores as raw fp64 bits, TP / FP / FN / TN -- except the ratio columns of the log (1e-12, as for GreConD).

Cases b, d and e end in the reference's own TypeError ("No pattern found"); the fixture keeps the rows and factors so far, which is
what the working stop leaves here.
"""
import contextlib
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
from scipy.sparse import csr_matrix

from grecondplus_ref import (CASES, COVERED, OVERLAPPED, NumpyExpansionEngine, check_fit, decide, expansion_ref, fit_case, line_counts,
                             line_scores, load_case, load_covered, load_overlapped, log_rows, numpy_engine, overlap_prefilter_ref,
                             remove_covered_ref, remove_overlapped_ref)
from test_grecond_cpu import FIT_KW, pack_rows, unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", CASES)
def test_host_loop_reproduces_the_reference(name):
    case = load_case(name)
    model = fit_case(case, numpy_engine)
    check_fit(model, case)
    rows = case["log"]["rows"]
    if name == "a":
        assert len(rows) == 5 and model.U.shape[1] == 5
    if name == "b":      # many factors, long expansions, factors swallowed by later ones, the k column repeats
        assert len(rows) == 65 and model.U.shape[1] == 49 and max(model.n_steps) > 40 and sum(model.n_covered) >= 16
        assert len(set(r[0] for r in rows)) < len(rows)
    if name == "c":      # with k given the first remove_covered() drops init_model's empty factors: 8 rows for k = 6
        assert [r[0] for r in rows] == [0, 1, 1, 1, 2, 3, 4, 5] and model.U.shape[1] == 4 and model.n_covered[0] == 5
    if name in ("b", "d"):
        assert case["raised"] == "TypeError" and model._engine.counts("train")[2] == 0       # ends with nothing left to cover
    if name == "e":
        assert rows == [] and model.U.shape == (20, 0) and model.U_exp.shape == (20, 0) and model.V_exp.shape == (15, 0)
    if name == "g":
        assert [c.split("/")[0] for c in case["log"]["columns"][4:]] == ["train"] * 4 + ["val"] * 4 + ["test"] * 4
    assert all(p == (0, 0, 0) or p[1:] == (0, 0) for p in model.n_pruned)     # no natural fit prunes an extension


def test_the_fixtures_hold_both_kinds_of_stop():
    tie = low = 0
    for name in CASES:
        t = load_case(name)["trace"]
        stops = t[t[:, 1] == -1]
        tie += int(((stops[:, 3] == stops[:, 4]) & (stops[:, 3] > 0)).sum())
        low += int(((stops[:, 3] <= 0) & (stops[:, 4] <= 0)).sum())
    assert tie >= 1 and low >= 1


@pytest.mark.parametrize("name", ["b", "c"])
def test_stand_in_counters_follow_the_definition(name):
    """The matrix-vector form of the stand-in's counters against the set definition, at every step of a long expansion."""
    case = load_case(name)
    X = case["X"] != 0
    rng = np.random.RandomState(3)
    RS = X & (rng.rand(*X.shape) < 0.5)
    u, v = np.zeros(X.shape[0], bool), np.zeros(X.shape[1], bool)
    u[:5], v[:4] = True, True
    w_fp, w_fn = 0.3, 0.7
    u_exp, v_exp, trace, counters = expansion_ref(X, RS, u, v, w_fp, w_fn, with_counters=True)
    assert len(trace) >= 3
    for (axis, index, r_score, c_score), (rows, cols) in zip(trace, counters):
        a, b, c = line_counts(X, RS, v)
        assert rows.tolist() == [a.tolist(), b.tolist(), c.tolist()]
        a, b, c = line_counts(X.T, RS.T, u)
        assert cols.tolist() == [a.tolist(), b.tolist(), c.tolist()]
        d = line_scores(*rows, u, w_fp, w_fn)
        assert r_score == d.max() and decide(r_score, c_score) == axis
        if axis == 1:
            assert index == int(np.argmax(d)) and not u[index]
            u[index] = True
        elif axis == 0:
            assert not v[index]
            v[index] = True
    assert (u_exp & ~u).sum() == 0 and (v_exp & ~v).sum() == 0


@pytest.mark.parametrize("name", OVERLAPPED)
def test_remove_overlapped_on_the_constructed_states(name):
    s = load_overlapped(name)
    out = remove_overlapped_ref(s["X"], s["U0"], s["V0"], s["Ue0"], s["Ve0"])
    for got, key in zip(out, ("U1", "V1", "Ue1", "Ve1")):
        assert got.tolist() == s[key].tolist(), key
    passed = overlap_prefilter_ref(s["X"], s["U0"], s["V0"], s["Ue0"], s["Ve0"])
    assert (passed > 0) == (name in ("row", "column", "stale", "twice", "single"))
    assert (s["rows_removed"], s["columns_removed"]) == {"row": (1, 0), "column": (0, 1), "stale": (1, 0), "twice": (1, 1)}.get(name, (0, 0))
    # through the engine's packed interface
    eng = NumpyExpansionEngine(s["X"])
    packed = eng.prune_overlapped(pack_rows(s["U0"].T, eng.W), pack_rows(s["V0"].T, eng.nvw), pack_rows(s["Ue0"].T, eng.W),
                                  pack_rows(s["Ve0"].T, eng.nvw))
    for got, key, length in zip(packed, ("U1", "V1", "Ue1", "Ve1"), (eng.m, eng.n, eng.m, eng.n)):
        assert [unpack(r, length).astype(int).tolist() for r in got] == s[key].T.tolist(), key
    assert eng.pruned == (passed, s["rows_removed"], s["columns_removed"])


@pytest.mark.parametrize("name", COVERED)
def test_remove_covered_on_the_constructed_states(name):
    s = load_covered(name)
    out = remove_covered_ref(s["U0"], s["V0"], s["Ue0"], s["Ve0"], s["k"])
    for got, key in zip(out, ("U1", "V1", "Ue1", "Ve1")):
        assert got.shape == s[key].shape and got.tolist() == s[key].tolist(), key
    assert out[0].shape[1] == s["kept"]


def test_steps_and_block_do_not_change_the_host_loop():
    case = load_case("c")
    ref = fit_case(case, numpy_engine)
    model = fit_case(case, numpy_engine, steps=3, block=5)
    assert log_rows(model) == log_rows(ref) and model.traces == ref.traces
    check_fit(model, case)


def test_parameter_checks_and_refusals():
    from pybmf_amd.models import GreConDPlus
    case = load_case("a")
    X = csr_matrix(case["X"].astype(np.float64))
    with contextlib.redirect_stdout(io.StringIO()):
        model = GreConDPlus()
        assert (model.k, model.tol, model.w_fp, model.w_fn) == (None, 0, 0.5, None)
        for bad in (dict(w_fp=float("nan")), dict(w_fp=None), dict(w_fp="0.5"), dict(w_fn=float("inf")), dict(k=0), dict(k=2.5)):
            with pytest.raises(ValueError):
                GreConDPlus(**bad)
        with pytest.raises(ValueError, match="steps"):
            GreConDPlus(k=2).fit(X, **dict(FIT_KW, steps=0))
        with pytest.raises(NotImplementedError, match="reconstruction"):
            GreConDPlus(k=2).fit(X, **dict(FIT_KW, task="prediction"))
        with pytest.raises(NotImplementedError, match="Boolean"):
            GreConDPlus(k=2).fit(case["X"].astype(np.float64) * 3, **FIT_KW)
        with pytest.raises(NotImplementedError, match="Boolean"):
            GreConDPlus(k=2).fit(X, X_val=X * 2, **FIT_KW)


# ---- ABI --------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = {"bmf_expand_counts": 7, "bmf_expand_rec_words": 2, "bmf_expand_steps": 19, "bmf_bits_rebuild": 12, "bmf_bits_subset": 10,
                    "bmf_overlap_counts": 10, "bmf_overlap_prune": 13}


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
        assert len(args) == n_args and res is (L._i64 if name.endswith("_words") else C.c_int)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from pybmf_amd import _lib as L
    lib = L.lib
    buf = (C.c_int64 * 4096)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)
    assert lib.bmf_expand_rec_words(0, 5) == -1 and lib.bmf_expand_rec_words(96, 72) == 4 + 4 * (96 + 72 + 1)
    assert lib.bmf_expand_counts(None, p, 4, 16, p, p, None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert lib.bmf_expand_counts(p, p, 4, 6, p, p, None) == -1 and b"multiple of 4" in lib.bmf_last_error()
    assert lib.bmf_expand_counts(p, odd, 4, 16, p, p, None) == -1 and b"16-byte" in lib.bmf_last_error()
    assert lib.bmf_expand_counts(p, p, 0, 16, p, p, None) == -1
    ok = [p, p, p, p, 4, 4, 16, 16, 0.5, 0.5, 1, p, p, p, p, p, p, p, None]

    def steps(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.bmf_expand_steps(*a)
    assert steps(a17=None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert steps(a10=0) == -1                                                   # no steps
    assert steps(a4=600) == -1 and b"ldw" in lib.bmf_last_error()               # m rows do not fit 16 words
    assert steps(a8=float("nan")) == -1 and b"finite" in lib.bmf_last_error()
    assert steps(a9=float("inf")) == -1 and b"finite" in lib.bmf_last_error()
    assert steps(a17=odd) == -1 and b"aligned" in lib.bmf_last_error()
    assert lib.bmf_bits_rebuild(p, 4, 16, None, None, 16, 2, p, p, p, p, None) == -1       # factors without their sets
    assert lib.bmf_bits_rebuild(p, 4, 16, p, p, 16, 2, p, None, p, p, None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert lib.bmf_bits_rebuild(p, 600, 16, p, p, 16, 2, p, p, p, p, None) == -1           # 600 lines do not fit 16 member words
    assert lib.bmf_bits_rebuild(p, 4, 16, p, p, 16, 2, p, p, None, p, None) == -1          # a sum without counts
    assert lib.bmf_bits_subset(p, 4, 16, p, 2, p, None, 3, p, None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert lib.bmf_bits_subset(p, 4, 16, p, 2, p, p, 0, p, None) == -1
    assert lib.bmf_overlap_counts(p, 16, p, 16, 2, 4, 4, None, 4, None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert lib.bmf_overlap_counts(p, 16, p, 16, 2, 4, 40, p, 4, None) == -1 and b"ldc" in lib.bmf_last_error()
    assert lib.bmf_overlap_prune(p, 16, 4, 4, p, 4, p, p, p, p, None, 16, None) == -1 and b"null pointer" in lib.bmf_last_error()
    assert lib.bmf_overlap_prune(p, 16, 4, 4, p, 4, p, p, p, p, p, 16, None) == -1 and b"copy of u" in lib.bmf_last_error()
    assert lib.bmf_overlap_prune(p, 16, 4, 4, p, 2, odd, p, p, p, p, 16, None) == -1 and b"ldc" in lib.bmf_last_error()
