"""PNLPF and WNMF with the Kullback-Leibler loss at a rank 64 < k <= 128 through the classes: every case of the reference golden g35
(tests/golden/make_golden_link_wide.py) at the gates tests/test_link_gpu.py holds k <= 64 to, the classes against the oracle at
k = 100, and a k = 6 fit against its g10 expectations (the rank picker leaves k <= 64 on the engines it had)."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle as orc  # noqa: E402

FIT = dict(show_logs=False, show_result=False, save_model=False)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@contextlib.contextmanager
def quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


def relf(a, b):
    return np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) / np.linalg.norm(np.asarray(b, dtype=np.float64))


def frame_values(df):
    return np.array([[float(v) for v in row[1:]] for row in df.values.tolist()])


def worst(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


@pytest.fixture(scope="module")
def g35(golden_dir):
    z = np.load(os.path.join(golden_dir, "g35_link_wide.npz"))
    meta = json.load(open(os.path.join(golden_dir, "g35_link_wide.json")))
    return z, meta


def dense(z, name):
    n = int(z["shape"][1])
    return np.unpackbits(z[f"{name}_X"], axis=1)[:, :n].astype(np.float64)


def cells(z, prefix):
    from scipy.sparse import csr_matrix
    m, n = (int(v) for v in z["shape"])
    X = csr_matrix((z[prefix + "_vals"].astype(np.float64), (z[prefix + "_rows"], z[prefix + "_cols"])), shape=(m, n))
    assert X.nnz == len(z[prefix + "_rows"])      # explicit zeros stay stored
    return X


def check_pnlpf(mdl, z, c, name):
    print(f"g35 {name}: PNLPF k={c['k']} W={c['W']} {c['task']}: relf U {relf(mdl.U, z[name + '_U']):.2e} V {relf(mdl.V, z[name + '_V']):.2e}, "
          f"largest entry deviation U {worst(mdl.U, z[name + '_U']):.2e} V {worst(mdl.V, z[name + '_V']):.2e}")
    assert type(mdl._eng).__module__ in ("pybmf_amd.link_wide", "pybmf_amd.wide")
    assert relf(mdl.U, z[name + "_U"]) < 1e-4 and relf(mdl.V, z[name + "_V"]) < 1e-4
    np.testing.assert_allclose(frame_values(mdl.logs["updates"]), np.array(c["updates"]["rows"]), rtol=1e-4)
    np.testing.assert_allclose(frame_values(mdl.logs["boolean"]), np.array(c["boolean"]["rows"]), rtol=1e-12, atol=0)
    assert float(mdl.reg) == pytest.approx(c["final_reg"], rel=1e-12)


def pnlpf_of(z, meta, name):
    from pybmf_amd.models import PNLPF
    c, p = meta["cases"][name], meta["pnlpf"]
    return c, PNLPF(k=c["k"], U=z[name + "_U0"].copy(), V=z[name + "_V0"].copy(), W=c["W"], reg=p["reg"], reg_growth=p["reg_growth"],
                    link_lamda=p["link_lamda"], init_method="custom", normalize_method=None, max_iter=p["max_iter"])


@pytest.mark.parametrize("name", ["a", "c"])
def test_pnlpf_full_mask_matches_reference(g35, name):
    z, meta = g35
    c, mdl = pnlpf_of(z, meta, name)
    with quiet():
        mdl.fit(dense(z, name), task="reconstruction", **FIT)
    check_pnlpf(mdl, z, c, name)


def test_pnlpf_prediction_with_val_and_test_sets_matches_reference(g35):
    z, meta = g35
    c, mdl = pnlpf_of(z, meta, "b")
    with quiet():
        mdl.fit(cells(z, "b_train"), cells(z, "b_val"), cells(z, "b_test"), task="prediction", **FIT)
    cols = [tuple(str(x) for x in col) for col in mdl.logs["updates"].columns][1:]
    assert cols == [tuple(x) for x in c["updates"]["columns"]]
    check_pnlpf(mdl, z, c, "b")


def test_pnlpf_under_a_mask_and_single_steps_match_reference(g35):
    from pybmf_amd.models.PNLPF import update_U, update_V
    z, meta = g35
    c, mdl = pnlpf_of(z, meta, "d")
    with quiet():
        mdl.fit(cells(z, "d"), task="reconstruction", **FIT)
    check_pnlpf(mdl, z, c, "d")
    Xd, Wr = dense(z, "d").astype(np.uint8), z["d_Wr_levels"].astype(np.float64) / 2
    for i, st in enumerate(c["steps"]):
        Vn = update_V(Xd, Wr, z["d_U0"], z["d_V0"], st["reg"], st["link_lamda"])
        Un = update_U(Xd, Wr, z["d_U0"], z[f"d_step{i}_V"].astype(np.float64), st["reg"], st["link_lamda"])
        print(f"g35 d step {i}: relf V {relf(Vn, z[f'd_step{i}_V']):.2e} U {relf(Un, z[f'd_step{i}_U']):.2e}, largest entry deviation "
              f"V {worst(Vn, z[f'd_step{i}_V']):.2e} U {worst(Un, z[f'd_step{i}_U']):.2e}")
        assert relf(Vn, z[f"d_step{i}_V"]) < 1e-5 and relf(Un, z[f"d_step{i}_U"]) < 1e-5


@pytest.mark.parametrize("name", ["e", "f", "g"])
def test_wnmf_kl_matches_reference(g35, name):
    from pybmf_amd.models import WNMF
    z, meta = g35
    c = meta["cases"][name]
    start = c["start"]
    X = dense(z, start)
    W = {"full": "full", "mask": "mask", "weights": None}[c["W"]]
    if W is None:
        W = z["g_Wr_levels"].astype(np.float64) / 2
    with quiet():
        w = WNMF(k=c["k"], U=z[start + "_U0"].copy(), V=z[start + "_V0"].copy(), W=W, beta_loss="kullback-leibler", init_method="custom",
                 max_iter=meta["kl_max_iter"])
        w.fit(X.copy(), task="reconstruction", **FIT)
    print(f"g35 {name}: WNMF-KL k={c['k']} W={c['W']}: relf U {relf(w.U, z[name + '_U']):.2e} V {relf(w.V, z[name + '_V']):.2e}, "
          f"largest entry deviation U {worst(w.U, z[name + '_U']):.2e} V {worst(w.V, z[name + '_V']):.2e}")
    assert type(w._eng).__name__ == {"e": "WideLinkMUEngine", "f": "WideLinkMUEngine", "g": "WideMaskedMUEngine"}[name]
    if name == "f":
        assert w._eng.obs_bits is not None       # the default mask on a dense matrix: the objective over the non-zeros of X
    assert relf(w.U, z[name + "_U"]) < 1e-4 and relf(w.V, z[name + "_V"]) < 1e-4
    np.testing.assert_allclose(frame_values(w.logs["updates"]), np.array(c["updates"]["rows"]), rtol=1e-4)


@pytest.mark.parametrize("task", ["reconstruction", "prediction"])
def test_val_and_test_sets_are_scored_at_the_wide_rank(g35, task):
    """fit(X_train, X_val, X_test) at k = 72 on the split of case b: the last log row's val / test columns are the oracle's scores of the
    model's own final factors -- whole matrices under 'reconstruction' (WholeScorer: bmf_link_sums_wide for PNLPF's link prediction),
    the sets' entries under 'prediction' (ObservedScorer: the sums of bmf_masked_link_pass_wide); WNMF-KL scores U V^T."""
    from pybmf_amd.models import PNLPF, WNMF
    z, meta = g35
    sets = {nm: cells(z, "b_" + nm) for nm in ("train", "val", "test")}
    with quiet():
        p = PNLPF(k=72, U=z["b_U0"].copy(), V=z["b_V0"].copy(), W="mask", reg=1.0, reg_growth=1.2, link_lamda=10, init_method="custom",
                  normalize_method=None, max_iter=2)
        p.fit(sets["train"].copy(), sets["val"].copy(), sets["test"].copy(), task=task, **FIT)
        w = WNMF(k=72, U=z["b_U0"].copy(), V=z["b_V0"].copy(), W="mask", beta_loss="kullback-leibler", init_method="custom", max_iter=2)
        w.fit(sets["train"].copy(), sets["val"].copy(), sets["test"].copy(), task=task, **FIT)
    for mdl, pred in ((p, orc.pnlpf_prediction(p.U, p.V, 10)), (w, w.U @ w.V.T)):
        cols = [tuple(str(x) for x in c) for c in mdl.logs["updates"].columns]
        row = mdl.logs["updates"].values.tolist()[-1]
        for nm in ("val", "test"):
            coo = sets[nm].tocoo()
            if task == "reconstruction":
                want = orc.rmse_mae(sets[nm].toarray(), pred)
            else:      # the non-zero entries of the set (the continuous models densify their data sets: ContinuousModel._make_scorers)
                keep = coo.data != 0
                d = coo.data[keep] - pred[coo.row[keep], coo.col[keep]]
                want = float(np.sqrt((d ** 2).mean())), float(np.abs(d).mean())
            got = float(row[cols.index((nm, "0", "RMSE"))]), float(row[cols.index((nm, "0", "MAE"))])
            print(f"{type(mdl).__name__} k=72 {task} {nm}: RMSE {got[0]:.6f} (oracle {want[0]:.6f}) MAE {got[1]:.6f} (oracle {want[1]:.6f})")
            assert got[0] == pytest.approx(want[0], rel=1e-5) and got[1] == pytest.approx(want[1], rel=1e-5)


def test_classes_against_the_oracle_at_k_100():
    """A rank between the fixture's: 36 real columns in the second block, three row blocks one way, two the other, two updates."""
    from pybmf_amd.models import PNLPF, WNMF
    from pybmf_amd.models.PNLPF import update_U, update_V
    m, n, k = 290, 150, 100
    rs = np.random.RandomState(100)
    X = (rs.rand(m, n) < 0.3).astype(np.float64)
    s = np.sqrt(0.5 / k) / 0.8
    U0 = np.abs(rs.standard_normal((m, k))) * s + 1e-3
    V0 = np.abs(rs.standard_normal((n, k))) * s + 1e-3
    ref = orc.pnlpf_fit(X, k=k, U=U0.copy(), V=V0.copy(), reg=1.0, link_lamda=10, reg_growth=1.2, init_method="custom", normalize_method=None,
                        max_iter=1, tol=-1.0)
    with quiet():
        p = PNLPF(k=k, U=U0.copy(), V=V0.copy(), W="full", reg=1.0, link_lamda=10, reg_growth=1.2, init_method="custom", normalize_method=None,
                  max_iter=1, tol=-1.0)
        p.fit(X.copy(), task="reconstruction", **FIT)
    print(f"k=100 PNLPF: relf U {relf(p.U, ref['U']):.2e} V {relf(p.V, ref['V']):.2e}")
    assert type(p._eng).__name__ == "WideLinkMUEngine"
    assert relf(p.U, ref["U"]) < 2e-5 and relf(p.V, ref["V"]) < 2e-5
    np.testing.assert_allclose(frame_values(p.logs["updates"]), np.array(ref["updates"]), rtol=1e-4)
    near = min(np.abs(np.asarray(ref["U"]) - 0.5).min(), np.abs(np.asarray(ref["V"]) - 0.5).min())
    if near > 1e-4:       # (the counts are decided only if no entry sits at the threshold)
        np.testing.assert_allclose(frame_values(p.logs["boolean"]), np.array(ref["boolean"]), rtol=1e-12)
    V1 = update_V(X, None, U0, V0, 1.0, 10)
    assert relf(V1, orc.pnlpf_update_V(X, None, U0, V0, 1.0, 10)) < 5e-6
    U1 = update_U(X, None, U0, V1, 1.0, 10)
    assert relf(U1, orc.pnlpf_update_U(X, None, U0, V1, 1.0, 10)) < 5e-6
    refk = orc.wnmf_kl_fit(X.copy(), k, U=U0.copy(), V=V0.copy(), W=None, max_iter=1, init_method="custom")
    with quiet():
        w = WNMF(k=k, U=U0.copy(), V=V0.copy(), W="full", beta_loss="kullback-leibler", init_method="custom", max_iter=1)
        w.fit(X.copy(), task="reconstruction", **FIT)
    print(f"k=100 WNMF-KL: relf U {relf(w.U, refk['U']):.2e} V {relf(w.V, refk['V']):.2e}")
    assert relf(w.U, refk["U"]) < 2e-5 and relf(w.V, refk["V"]) < 2e-5
    np.testing.assert_allclose(frame_values(w.logs["updates"]), np.array(refk["updates"]), rtol=1e-4)


def test_class_refusals_on_the_device():
    from pybmf_amd.models import PNLPF, WNMF
    rs = np.random.RandomState(1)
    X = (rs.rand(40, 30) < 0.3).astype(np.uint8)
    with quiet():
        with pytest.raises(NotImplementedError, match=r"^k=129: this build supports k <= 128$"):
            PNLPF(k=129, U=rs.rand(40, 129), V=rs.rand(30, 129), W="full", max_iter=2).fit(X, task="reconstruction", **FIT)
        with pytest.raises(NotImplementedError, match=r"^k=129: this build supports k <= 128$"):
            WNMF(k=129, U=rs.rand(40, 129), V=rs.rand(30, 129), W="full", beta_loss="kullback-leibler", init_method="custom",
                 max_iter=2).fit(X, task="reconstruction", **FIT)
        with pytest.raises(NotImplementedError, match="k=70.*Boolean"):
            WNMF(k=70, U=rs.rand(40, 70), V=rs.rand(30, 70), W="full", beta_loss="kullback-leibler", init_method="custom",
                 max_iter=2).fit(rs.rand(40, 30), task="reconstruction", **FIT)
        with pytest.raises(NotImplementedError, match="k=70.*Boolean"):
            PNLPF(k=70, U=rs.rand(40, 70), V=rs.rand(30, 70), W="full", max_iter=2).fit(rs.rand(40, 30), task="reconstruction", **FIT)


def test_a_rank_of_6_stays_on_the_narrow_engine(golden_dir):
    """k <= 64 is untouched: the same engine class, and the g10 expectations at the gates of tests/test_link_gpu.py."""
    from pybmf_amd.models import PNLPF, WNMF
    z = np.load(os.path.join(golden_dir, "g10_link_models.npz"))
    meta = json.load(open(os.path.join(golden_dir, "g10_link_models.json")))
    n = int(z["shape"][1])
    X = np.unpackbits(z["X"], axis=1)[:, :n].astype(np.float64)
    p = meta["pnlpf"]["params"]
    with quiet():
        mdl = PNLPF(k=p["k"], U=z["p_U0"].copy(), V=z["p_V0"].copy(), W="full", reg=p["reg"], reg_growth=p["reg_growth"],
                    link_lamda=p["link_lamda"], init_method="custom", normalize_method=None, max_iter=p["max_iter"])
        mdl.fit(X.copy(), task="reconstruction", **FIT)
        w = WNMF(k=6, U=z["w_U0"].copy(), V=z["w_V0"].copy(), W="full", beta_loss="kullback-leibler", init_method="custom", max_iter=9)
        w.fit(X.copy(), task="reconstruction", **FIT)
    assert type(mdl._eng).__name__ == "LinkMUEngine" and type(w._eng).__name__ == "LinkMUEngine" and mdl._eng.mfma == "bf16"
    assert relf(mdl.U, z["p_U"]) < 1e-4 and relf(mdl.V, z["p_V"]) < 1e-4
    np.testing.assert_allclose(frame_values(mdl.logs["updates"]), np.array(meta["pnlpf"]["updates"]["rows"]), rtol=1e-4)
    np.testing.assert_allclose(frame_values(mdl.logs["boolean"]), np.array(meta["pnlpf"]["boolean"]["rows"]), rtol=1e-12, atol=0)
    assert float(mdl.reg) == pytest.approx(meta["pnlpf"]["final_reg"], rel=1e-12)
    assert relf(w.U, z["w_U"]) < 1e-4 and relf(w.V, z["w_V"]) < 1e-4
    np.testing.assert_allclose(frame_values(w.logs["updates"]), np.array(meta["wnmf_kl"]["updates"]["rows"]), rtol=1e-4)
