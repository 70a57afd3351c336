"""Rank 65-128 of the proximal models without a GPU: the fixture g34 (tests/golden/make_golden_palm_wide.py) is consistent with itself
and keeps the margins its generator promises, and the two new entry points are declared, exported and bound with matching types."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "bmf_hip.h")


@pytest.fixture(scope="module")
def g34():
    z = np.load(os.path.join(GOLDEN, "g34_palm_wide.npz"))
    steps = np.load(os.path.join(GOLDEN, "g34_palm_wide_steps.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "g34_palm_wide.json")))
    return z, steps, meta


def loop_cases(meta):
    for k in meta["ks"]:
        for name, g in meta[f"k{k}"].items():
            if isinstance(g, dict) and "updates" in g:
                yield k, name, g


def test_fixture_files_are_small_and_hold_data_only():
    for f in ("g34_palm_wide.npz", "g34_palm_wide_steps.npz", "g34_palm_wide.json"):
        assert os.path.getsize(os.path.join(GOLDEN, f)) < (1 << 20), f
    for f in ("g34_palm_wide.npz", "g34_palm_wide_steps.npz"):
        with np.load(os.path.join(GOLDEN, f), allow_pickle=False) as z:
            assert all(z[n].dtype.kind in "fiu" for n in z.files)


def test_fixture_json_and_npz_agree(g34):
    z, steps, meta = g34
    assert meta["ks"] == [65, 72, 128] and meta["margin"] == 1e-3 and meta["jitter_tol"] == 1e-5
    seen = set()
    for k, name, g in loop_cases(meta):
        seen.add((k, name))
        m, n, kk = meta[f"k{k}"]["shape"]
        assert (m, n, kk) == (3 * k, 2 * k, k)
        X = np.unpackbits(z[f"k{k}_X"], axis=1)[:, :n].astype(np.float64)
        if name in ("mpalm", "mipalm"):   # W='mask': the training matrix is the csr of the observed cells, the rest reads as 0
            X = X * np.unpackbits(z["k72_W01"], axis=1)[:, :n]
        assert X.shape == (m, n) and z[f"k{k}_U0_grid"].shape == (m, k) and z[f"k{k}_V0_grid"].shape == (n, k) and z[f"k{k}_U0_grid"].dtype == np.uint8
        U, V = z[f"k{k}_{name}_U"].astype(np.float64), z[f"k{k}_{name}_V"].astype(np.float64)
        assert U.shape == (m, k) and V.shape == (n, k)
        rows = np.array(g["updates"]["rows"], dtype=np.float64)
        assert rows.shape == (g["n_iter"], 12) and np.array_equal(rows[:, 0], np.arange(g["n_iter"]))
        # the recorded counts and scores are those of the recorded factors (no entry is near the threshold: fp32 storage cannot flip one)
        cnt = orc.confusion_counts(X.astype(np.int64), orc.boolean_product(U, V, 0.5, 0.5))
        assert list(cnt) == g["counts"] and sum(g["counts"]) == m * n
        rec, prec, acc, f1 = orc.boolean_scores(*cnt)
        np.testing.assert_allclose(rows[-1, 7:], [1 - acc, acc, rec, prec, f1], rtol=1e-12, atol=1e-15)
        # ... and so are the logged error and gaps (to the fp32 storage of the factors)
        assert rows[-1, 6] == pytest.approx(float(((X - U @ V.T) ** 2).sum()), rel=1e-5)
        l1, l2 = rows[-1, 1], rows[-1, 2]
        assert l2 == pytest.approx(meta["loop"]["reg_l2"] * meta["loop"]["reg_growth"] ** (g["n_iter"] - 1), rel=1e-12)
        assert rows[-1, 4] == pytest.approx(orc.elbmf_integrality_gap(U, l1, l2), rel=1e-5) and rows[-1, 3] == pytest.approx(rows[-1, 4] + rows[-1, 5], rel=1e-12)
    assert seen == {(k, t) for k in (65, 72, 128) for t in ("palm", "ipalm")} | {(72, "mpalm"), (72, "mipalm"), (72, "stop")}
    m, n = 216, 144
    assert z["k72_U_prev_grid"].shape == (m, 72) and z["k72_U_prev_grid"].dtype == np.int16 and np.abs(z["k72_U_prev_grid"]).max() == 128
    assert z["k72_W01"].shape == (m, n // 8) and set(np.unique(z["k72_Wr_levels"])) == {0, 1, 2, 4}
    W01 = np.unpackbits(z["k72_W01"], axis=1)[:, :n]
    assert np.array_equal(z["k72_Wr_levels"] > 0, W01 > 0) and not W01[7].any() and not W01[:, 11].any()
    assert len(meta["steps"]) == 4 and len(meta["masked_steps"]) == 4 and len(meta["primp_steps"]) == 3
    for i in range(4):
        for pre in ("step", "mstep"):
            assert steps[f"k72_{pre}{i}_U"].shape == (m, 72) and steps[f"k72_{pre}{i}_V"].shape == (n, 72)
    assert all(steps[f"k72_pstep{i}_U"].shape == (m, 72) for i in range(3))
    for tag in ("primp64", "primp64_b0"):
        U, Vt = z[f"k72_{tag}_U"].astype(np.float64), z[f"k72_{tag}_Vt"].astype(np.float64)
        X = np.unpackbits(z["k72_X"], axis=1)[:, :n].astype(np.float64)
        assert meta[tag]["fn_final"] == pytest.approx(float(((X - U @ Vt) ** 2).sum()), rel=1e-5)
        far = np.abs(U - 0.5) > 1e-4
        assert np.array_equal(np.unpackbits(z[f"k72_{tag}_Ur"], axis=1)[:, :72].astype(bool)[far], (U > 0.5)[far])
    assert z["k72_primp_seed3_U0"].shape == (m, 72) and z["k72_primp_seed3_Vt0"].shape == (72, n) and z["k72_primp_seed3_U0"].dtype == np.float32


def test_fixture_keeps_its_margins(g34):
    z, _, meta = g34
    for k, name, g in loop_cases(meta):
        assert g["min_dist_to_half"] >= meta["margin"], (k, name)
        assert g["jitter_moved"] <= meta["jitter_tol"], (k, name)
        U, V = z[f"k{k}_{name}_U"].astype(np.float64), z[f"k{k}_{name}_V"].astype(np.float64)
        assert min(np.abs(U - 0.5).min(), np.abs(V - 0.5).min()) >= meta["margin"] * 0.999       # (the final iterate, as stored)
    g = meta["k72"]["stop"]
    rows = np.array(g["updates"]["rows"], dtype=np.float64)
    d = np.abs(np.diff(rows[:, 3]))
    assert g["n_iter"] == g["stop_iter"] + 1 < g["max_iter"]
    assert d[-1] <= 0.95 * g["min_diff"] and (d[:-1] >= 1.05 * g["min_diff"]).all()
    assert d[-1] == pytest.approx(g["diff_at_stop"], rel=1e-12) and d[-2] == pytest.approx(g["diff_before"], rel=1e-12)
    for k in meta["ks"]:   # the loops that do not stop early run max_iter + 2 updates
        assert all(meta[f"k{k}"][t]["n_iter"] == meta[f"k{k}"][t]["max_iter"] + 2 for t in ("palm", "ipalm"))


# ---- the two new entry points -----------------------------------------------------------------------------------------------------------
CTYPE_OF = {"const double*": C.c_void_p, "double*": C.c_void_p, "void*": C.c_void_p}


def declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in bmf_hip.h"
    return [re.sub(r"\s+", " ", re.sub(r"\b\w+$", "", a.strip()).strip()) for a in m.group(1).split(",")]


def test_new_symbols_are_declared_exported_and_bound_alike():
    from pybmf_amd import _lib as L
    raw = C.CDLL(L.LIB_PATH)
    assert hasattr(raw, "bmf_sym_norms_wide") and hasattr(raw, "bmf_palm_epilogue_wide")
    args = declaration("bmf_sym_norms_wide")
    assert args == ["const double*", "double*", "void*"]
    assert L.SIGNATURES["bmf_sym_norms_wide"] == (C.c_int, [CTYPE_OF[a] for a in args])
    args = declaration("bmf_palm_epilogue_wide")
    assert args == ["const bmf_palm_wide_args*", "void*"]
    res, bound = L.SIGNATURES["bmf_palm_epilogue_wide"]
    assert res is C.c_int and bound[0] is C.POINTER(L.PalmWideArgs) and bound[1] is C.c_void_p and len(bound) == 2
    # the struct's index in bmf_struct_bytes is appended: the existing ones keep theirs
    assert L.lib.bmf_struct_bytes(9) == C.sizeof(L.PalmWideArgs) and L.lib.bmf_struct_bytes(1) == C.sizeof(L.PalmArgs) and L.lib.bmf_struct_bytes(10) == -1


def test_wide_args_layout_matches_c(tmp_path):
    from pybmf_amd import _lib as L
    fields = ["rows_pad", "F64", "num", "G", "norms", "beta", "advance_prev", "thr", "rowbits", "ldcb", "partials"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(bmf_palm_wide_args));\n%s\nreturn 0;}\n'
                   % (HEADER, "\n".join('printf(" %%zu", offsetof(bmf_palm_wide_args, %s));' % f for f in fields)))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(L.PalmWideArgs)] + [getattr(L.PalmWideArgs, f).offset for f in fields]


def test_wide_entry_points_refuse_bad_arguments_without_a_gpu():
    from pybmf_amd import _lib as L
    lib = L.lib
    assert lib.bmf_sym_norms_wide(None, None, None) == -1 and b"bmf_sym_norms_wide: null pointer" in lib.bmf_last_error()
    assert lib.bmf_palm_epilogue_wide(None, None) == -1 and b"null args" in lib.bmf_last_error()
    a = L.PalmWideArgs()
    assert lib.bmf_palm_epilogue_wide(C.byref(a), None) == -1 and b"struct_bytes" in lib.bmf_last_error()
    a.struct_bytes = C.sizeof(L.PalmWideArgs)
    assert lib.bmf_palm_epilogue_wide(C.byref(a), None) == -1 and b"null pointer" in lib.bmf_last_error()
    junk = (C.c_double * 4)()
    p = C.addressof(junk)
    for b in range(2):
        a.F64[b] = a.Fprev64[b] = a.F[b] = a.num[b] = a.rowbits[b] = a.colbits[b] = a.partials[b] = p
        a.G[b][0] = a.G[b][1] = p
    a.norms = p
    a.rows_pad, a.rows, a.splits, a.slab_stride, a.ldcb, a.variant = 256, 130, 1, 256 * 64, 8, L.PALM_ELBMF
    for k in (64, 129, 0):     # k <= 64 belongs to bmf_palm_epilogue, k > 128 to nobody
        a.k = k
        assert lib.bmf_palm_epilogue_wide(C.byref(a), None) == -1 and b"64 < k <= 128" in lib.bmf_last_error(), k
    a.k, a.rows_pad = 72, 200
    assert lib.bmf_palm_epilogue_wide(C.byref(a), None) == -1 and b"multiple of 128" in lib.bmf_last_error()
    a.rows_pad, a.beta = 256, 1.0
    assert lib.bmf_palm_epilogue_wide(C.byref(a), None) == -1 and b"beta" in lib.bmf_last_error()


def test_engine_picker_refuses_by_rank_without_a_gpu():
    from pybmf_amd import _lib as L
    from pybmf_amd.palm_wide import palm_engine
    with pytest.raises(NotImplementedError, match="k <= 128"):
        palm_engine(None, 129, L.PALM_ELBMF)
    with pytest.raises(NotImplementedError, match="one GPU"):
        palm_engine(None, 72, L.PALM_ELBMF, sharded=True)
