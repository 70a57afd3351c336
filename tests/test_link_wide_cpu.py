"""The link models (PNLPF, WNMF with the Kullback-Leibler loss) at a rank 64 < k <= 128, the parts that need no GPU: the refusals of
the three entry points of csrc/link_wide.hip and of the engine picker, the margins the fixture g35 records
(tests/golden/make_golden_link_wide.py), and the fixture against the CPU oracle."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle as orc


@pytest.fixture(scope="module")
def g35(golden_dir):
    z = np.load(os.path.join(golden_dir, "g35_link_wide.npz"))
    meta = json.load(open(os.path.join(golden_dir, "g35_link_wide.json")))
    return z, meta


def last_error(lib):
    return lib.bmf_last_error().decode()


def relf(a, b):
    return np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) / np.linalg.norm(np.asarray(b, dtype=np.float64))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound():
    from pybmf_amd import _lib as L
    raw = C.CDLL(L.LIB_PATH)
    for name in ("bmf_link_pass_wide", "bmf_link_sums_wide", "bmf_masked_link_pass_wide"):
        assert hasattr(raw, name) and name in L.SIGNATURES, name


def test_link_pass_wide_refusals():
    from pybmf_amd import _lib as L
    lib = L.lib
    buf = (C.c_double * 66)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)      # 16-byte aligned, like every device allocation
    rows, cols = 130, 700
    splits = lib.bmf_link_splits(rows, cols)
    assert splits == 2

    def call(X=p, s0=p, s1=p, o0=p, o1=p, n0=p, n1=p, d0=p, d1=p, k=72, link=L.LINK_SIGMOID, splits=splits, rows=rows, cols=cols, rows_pad=256,
             other_pad=768, ldx=24, stride=256 * 64):
        return lib.bmf_link_pass_wide(X, rows_pad, ldx, rows, cols, s0, s1, o0, o1, other_pad, k, link, 10.0, n0, n1, d0, d1, stride, splits, None)

    for kw in (dict(X=None), dict(s0=None), dict(s1=None), dict(o0=None), dict(o1=None), dict(n0=None), dict(n1=None)):
        assert call(**kw) == -1 and "bmf_link_pass_wide: null pointer" in last_error(lib), kw
    for kw in (dict(d0=None), dict(d1=None)):
        assert call(**kw) == -1 and "bmf_link_pass_wide: the sigmoid link needs both den buffers" in last_error(lib), kw
    assert call(k=64) == -1 and "bmf_link_pass_wide: k=64 " in last_error(lib) and "bmf_link_pass;" in last_error(lib)
    assert call(k=129) == -1 and "bmf_link_pass_wide: k=129 " in last_error(lib) and "k <= 128" in last_error(lib)
    for link in (0, 9):
        assert call(link=link) == -1 and f"bmf_link_pass_wide: link={link}" in last_error(lib)
    for bad in (splits - 1, splits + 1, 0):
        assert call(splits=bad) == -1 and f"bmf_link_pass_wide: splits={bad}, this shape needs {splits} (bmf_link_splits)" in last_error(lib)
    for kw in (dict(rows=0), dict(cols=0), dict(rows=257), dict(rows_pad=200)):
        assert call(**kw) == -1 and "bmf_link_pass_wide: bad rows/rows_pad" in last_error(lib), kw
    for kw in (dict(other_pad=672), dict(other_pad=700), dict(ldx=21)):
        assert call(**kw) == -1 and "bmf_link_pass_wide: other_pad / ldx do not cover cols" in last_error(lib), kw
    assert call(stride=256 * 64 - 1) == -1 and "bmf_link_pass_wide: slab_stride too small" in last_error(lib)
    off = C.c_void_p(p.value + 4)
    for kw in (dict(s0=off), dict(s1=off), dict(o0=off), dict(o1=off)):
        assert call(**kw) == -1 and "bmf_link_pass_wide: factors must be 16-byte aligned" in last_error(lib), kw


def test_link_sums_wide_refusals():
    from pybmf_amd import _lib as L
    lib = L.lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(X=p, u0=p, u1=p, v0=p, v1=p, sums=p, k=72, link=L.LINK_KL, m=130, n=100, m_pad=256, n_pad=128, ldx=4):
        return lib.bmf_link_sums_wide(X, m_pad, ldx, m, n, u0, u1, v0, v1, n_pad, k, link, 10.0, None, sums, None)

    for kw in (dict(X=None), dict(u0=None), dict(u1=None), dict(v0=None), dict(v1=None), dict(sums=None)):
        assert call(**kw) == -1 and "bmf_link_sums_wide: null pointer" in last_error(lib), kw
    assert call(k=64) == -1 and "bmf_link_sums_wide: k=64 " in last_error(lib) and "bmf_link_sums;" in last_error(lib)
    assert call(k=129) == -1 and "bmf_link_sums_wide: k=129 " in last_error(lib) and "k <= 128" in last_error(lib)
    for link in (0, 9):
        assert call(link=link) == -1 and f"bmf_link_sums_wide: link={link}" in last_error(lib)
    for kw in (dict(m=0), dict(n=0), dict(m=257), dict(m_pad=130), dict(n=129), dict(n_pad=100), dict(ldx=3)):
        assert call(**kw) == -1 and "bmf_link_sums_wide: bad shape" in last_error(lib), kw


def test_masked_link_pass_wide_refusals():
    from pybmf_amd import _lib as L
    lib = L.lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    names = ("ptr", "idx", "val", "seg_row", "seg_beg", "row_seg_ptr", "s0", "s1", "o0", "o1", "p0", "p1", "n0", "n1", "d0", "d1")

    def call(link=L.LINK_SIGMOID, rows=10, nseg=1, **kw):
        a = {nm: p for nm in names}
        a.update(kw)
        return lib.bmf_masked_link_pass_wide(a["ptr"], a["idx"], a["val"], None, rows, a["seg_row"], a["seg_beg"], nseg, a["row_seg_ptr"], a["s0"],
                                             a["s1"], a["o0"], a["o1"], a["p0"], a["p1"], a["n0"], a["n1"], a["d0"], a["d1"], None, link, 10.0, None)

    for nm in names:
        assert call(**{nm: None}) == -1 and "bmf_masked_link_pass_wide: null pointer" in last_error(lib), nm
    assert call(link=0) == -1 and "bmf_masked_link_pass_wide: link=0 is bmf_masked_pass_wide" in last_error(lib)
    assert call(link=9) == -1 and "bmf_masked_link_pass_wide: link=9" in last_error(lib)
    for kw in (dict(rows=0), dict(nseg=-1)):
        assert call(**kw) == -1 and "bmf_masked_link_pass_wide: rows must be positive" in last_error(lib), kw


def test_recorded_resource_report_has_no_scratch():
    """profiles/link_wide_resources.txt is the compiler's report for csrc/link_wide.hip: all seven kernels, ScratchSize 0 and no spills."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = open(os.path.join(root, "profiles", "link_wide_resources.txt")).read().splitlines()
    names = [ln.split("Function Name: ")[1] for ln in lines if "Function Name: " in ln]
    for kernel, count in (("link_pass_wide_kernel", 2), ("link_sums_wide_kernel", 2), ("masked_link_segments_wide_kernel", 2), ("masked_link_rows_wide_kernel", 1)):
        assert sum(kernel in nm for nm in names) == count, kernel
    assert len(names) == 7
    for key in ("ScratchSize [bytes/lane]: ", "SGPRs Spill: ", "VGPRs Spill: "):
        vals = [ln.split(key)[1] for ln in lines if key in ln]
        assert vals == ["0"] * 7, key
    src = open(os.path.join(root, "pybmf_amd", "csrc", "link_wide.hip")).read()
    assert src.count("__global__") == 4                      # three kernels templated on the link (two instances each) and the row sum


# ---- the classes ----------------------------------------------------------------------------------------------------------------------
def test_engine_picker_refuses_by_rank_without_a_gpu():
    from pybmf_amd import _lib as L
    from pybmf_amd.link_wide import link_engine
    for link, mode in ((L.LINK_SIGMOID, L.MODE_PENALTY), (L.LINK_KL, L.MODE_WNMF)):
        with pytest.raises(NotImplementedError, match=r"^k=129: this build supports k <= 128$"):
            link_engine(None, 129, link, mode)
        with pytest.raises(NotImplementedError, match="k=72.*one GPU"):
            link_engine(None, 72, link, mode, sharded=True)
        with pytest.raises(NotImplementedError, match="k=72.*Boolean"):
            link_engine(None, 72, link, mode, boolean=False)
        with pytest.raises(NotImplementedError, match="k=72.*mfma='bf16'"):
            link_engine(None, 72, link, mode, mfma="bf16")


def test_module_level_steps_refuse_a_rank_above_128_without_a_gpu():
    from pybmf_amd.models.PNLPF import update_U, update_V
    rs = np.random.RandomState(0)
    X = (rs.rand(20, 15) < 0.3).astype(np.uint8)
    U, V = rs.rand(20, 129), rs.rand(15, 129)
    for fn in (update_U, update_V):
        with pytest.raises(NotImplementedError, match=r"^k=129: this build supports k <= 128$"):
            fn(X, None, U, V, 1.0, 10)


def test_wide_engines_refuse_other_ranks_and_links_without_a_gpu():
    from pybmf_amd import _lib as L
    from pybmf_amd.link_wide import WideLinkMUEngine
    from pybmf_amd.wide import WideMaskedMUEngine
    for k in (64, 129):
        with pytest.raises(NotImplementedError, match=f"k={k}"):
            WideLinkMUEngine(None, k, L.LINK_SIGMOID, L.MODE_PENALTY)
    with pytest.raises(ValueError, match="link"):
        WideLinkMUEngine(None, 72, 0, L.MODE_PENALTY)
    with pytest.raises(NotImplementedError, match="link"):
        WideMaskedMUEngine(None, 72, L.MODE_PENALTY, bits=None, link=L.LINK_SIGMOID)
    with pytest.raises(NotImplementedError, match="link"):
        WideMaskedMUEngine(None, 72, L.MODE_PENALTY, bits=object(), link=9)


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
def test_fixture_is_small_and_holds_data_only(golden_dir):
    for f in ("g35_link_wide.npz", "g35_link_wide.json"):
        assert os.path.getsize(os.path.join(golden_dir, f)) < (1 << 20), f
    z = np.load(os.path.join(golden_dir, "g35_link_wide.npz"), allow_pickle=False)
    assert all(z[n].dtype.kind in "fiu" for n in z.files)


def test_fixture_cases_are_the_issue_s(g35):
    z, meta = g35
    want = {"a": ("PNLPF", 65, "full", "reconstruction"), "b": ("PNLPF", 72, "mask", "prediction"), "c": ("PNLPF", 128, "full", "reconstruction"),
            "d": ("PNLPF", 72, "mask", "reconstruction"), "e": ("WNMF-KL", 72, "full", "reconstruction"), "f": ("WNMF-KL", 128, "mask", "reconstruction"),
            "g": ("WNMF-KL", 72, "weights", "reconstruction")}
    assert {n: (c["model"], c["k"], c["W"], c["task"]) for n, c in meta["cases"].items()} == want
    assert meta["pnlpf"] == {"reg": 1.0, "reg_growth": 1.2, "link_lamda": 10, "max_iter": 4}
    m, n = (int(v) for v in z["shape"])
    for name, c in meta["cases"].items():
        assert len(c["updates"]["rows"]) == 6            # rows 0 .. 5: five iterations
        assert z[f"{name}_U"].shape == (m, c["k"]) and z[f"{name}_V"].shape == (n, c["k"]) and z[f"{name}_U"].dtype == np.float32
        if c["model"] == "PNLPF":
            assert z[f"{name}_U0"].shape == (m, c["k"]) and z[f"{name}_U0"].dtype == np.float64 and len(c["boolean"]["rows"]) == 6
    assert (z["d_vals"] == 0).any() and (z["d_vals"] == 1).any() and 3 not in z["d_rows"] and 8 not in z["d_cols"]
    cols = [tuple(x) for x in meta["cases"]["b"]["updates"]["columns"]]
    assert ("val", "0", "RMSE") in cols and ("test", "0", "MAE") in cols


def test_fixture_keeps_its_margins(g35):
    _, meta = g35
    assert meta["margin"] == 3e-4 and meta["gate"] == 1e-4 and meta["jitter"] == 1e-6
    for name in "abcd":
        c = meta["cases"][name]
        assert c["min_dist_to_half"] >= 3e-4, name
        assert c["jitter_moved"] < 1e-4 / 3, name
        assert 1 <= c["seeds_tried"] <= 4000


def dense(z, name):
    n = int(z["shape"][1])
    return np.unpackbits(z[f"{name}_X"], axis=1)[:, :n].astype(np.float64)


@pytest.mark.parametrize("name", ["a", "c"])
def test_oracle_replays_the_pnlpf_cases(g35, name):
    z, meta = g35
    c, p = meta["cases"][name], meta["pnlpf"]
    X, U0, V0 = dense(z, name), z[f"{name}_U0"], z[f"{name}_V0"]
    ref = orc.pnlpf_fit(X, k=c["k"], U=U0.copy(), V=V0.copy(), reg=p["reg"], link_lamda=p["link_lamda"], reg_growth=p["reg_growth"],
                        init_method="custom", normalize_method=None, max_iter=p["max_iter"], trace=True)
    np.testing.assert_allclose(np.array(ref["updates"]), np.array(c["updates"]["rows"]), rtol=1e-10)
    np.testing.assert_allclose(np.array(ref["boolean"]), np.array(c["boolean"]["rows"]), rtol=1e-12, atol=0)
    assert ref["reg"] == pytest.approx(c["final_reg"], rel=1e-12)
    assert relf(ref["U"], z[f"{name}_U"]) < 1e-7 and relf(ref["V"], z[f"{name}_V"]) < 1e-7      # (the fixture stores them as fp32)
    near = min(min(np.abs(U - 0.5).min(), np.abs(V - 0.5).min()) for U, V in ref["trace"])
    assert near == pytest.approx(c["min_dist_to_half"], rel=1e-6)


def test_oracle_replays_the_kl_case(g35):
    z, meta = g35
    c = meta["cases"]["e"]
    X = dense(z, "b")
    ref = orc.wnmf_kl_fit(X.copy(), c["k"], U=z["b_U0"].copy(), V=z["b_V0"].copy(), W=None, max_iter=meta["kl_max_iter"], init_method="custom")
    np.testing.assert_allclose(np.array(ref["updates"]), np.array(c["updates"]["rows"]), rtol=1e-10)
    assert relf(ref["U"], z["e_U"]) < 1e-7 and relf(ref["V"], z["e_V"]) < 1e-7
