"""The multiplicative-update driver (csrc/api.hip) by bytes: what strings the kernels of an iteration together -- gather_body /
gather_kernel, finalize_body / finalize_kernel, reduce_finalize_kernel, reduce_slabs_block_kernel and sweep()'s phases behind
bmf_penalty_update, _update_head, _update_xtu, _finalize and _run.  The kernels those launch have their own files; the reference here is
tests/driver_ref.py (proved in tests/test_driver_cpu.py), or the device's own intermediate buffers read back.

Every test drives a real MUEngine on a small BitMatrix and makes its state by overwriting the engine's tensors.  Outputs are pre-filled
with a marker, inputs must come back byte for byte, and a test named for a launch form first asserts that form from the library's own
numbers on this device -- it fails, it does not skip, when the device gives another form.

  B  bmf_penalty_finalize on hand-made dyadic states: the log row == the definition, GU == float32(U^T U), the stopping rule at its
     edges, the stop freeze of the row
  C  the slab sums behind _update_xtu (reduce_slabs_kernel, reduce_slabs_wide_kernel, reduce_slabs_block_kernel) and _run
     (reduce_finalize_kernel) == the sums of the slabs read back, in each kernel's order
  D  the gather (gather_kernel after _update_head, gather_body inside finalize after _run) == the partials read back
  E  the three forms of an iteration give the same bytes; after the stop every buffer is frozen, set to a stated value, or scratch
     (the table at bmf_penalty_state.stop in include/bmf_hip.h)
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import driver_ref as R  # noqa: E402

MARK = -7.25          # exactly representable in every type used below
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pybmf_amd import _lib as L
    from pybmf_amd import engine as E
    return L, E


# ----------------------------------------------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------------------------------------------
_DATA, _BITS = {}, {}
TERMS = {"i8": 3, "f16": 2, "bf16": 3}


def data(m, n, k):
    """(X uint8, U0, V0): a planted 0/1 matrix with noise and small positive factors -- made once per shape, never modified"""
    key = (m, n, k)
    if key not in _DATA:
        rs = np.random.RandomState(m * 7 + n * 3 + k)
        A, B = rs.rand(m, 4) < 0.25, rs.rand(n, 4) < 0.25
        X = ((A.astype(np.int32) @ B.astype(np.int32).T) > 0) ^ (rs.rand(m, n) < 0.03)
        s = 2.0 * np.sqrt(0.2 / k)
        _DATA[key] = (X.astype(np.uint8), 0.02 + s * rs.rand(m, k), 0.02 + s * rs.rand(n, k))
    return _DATA[key]


def bitmatrix(E, m, n, k):
    """one BitMatrix per shape, shared by every engine on it (the tests check that it comes back byte for byte)"""
    key = (m, n, k)
    if key not in _BITS:
        _BITS[key] = E.BitMatrix(data(m, n, k)[0], DEV)
    return _BITS[key]


def engine(gpu, m, n, k, panel="i8", prepare=1.0, **kw):
    L, E = gpu
    X, U0, V0 = data(m, n, k)
    kw.setdefault("tol", -1.0)
    kw.setdefault("max_iter", 12)
    eng = E.MUEngine(bitmatrix(E, m, n, k), k=k, mode=kw.pop("mode", L.MODE_PENALTY), panel=panel, terms=TERMS[panel], **kw)
    eng.load_factors(U0, V0)
    if prepare is not None:
        eng.prepare(prepare)
    return eng


def host(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def same(a, b):
    """byte for byte (so -0.0 != +0.0 and a NaN equals the same NaN)"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def ulps(a, b):
    """distance of two finite non-negative doubles in units in the last place"""
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


FROZEN = ("U64", "V64", "U", "V", "ubits", "vbits", "ucolbits", "vcolbits", "ubits_prev", "vbits_prev", "counts", "Upanel", "Vpanel",
          "scaleU", "scaleV", "GU", "GV", "scal", "log", "stop")
DERIVED = ("comm", "GV64")
SCRATCH = ("Mslab", "Nslab", "gram_slabs", "panel_ws", "partU", "partV", "_nred_flat", "mae_ws")


def snap(eng, names=FROZEN + DERIVED + SCRATCH):
    torch.cuda.synchronize()
    return {name: host(getattr(eng, name)) for name in names}


def x_bytes(eng):
    torch.cuda.synchronize()
    out = [host(eng.X.bits), host(eng.X.bits_t)]
    if getattr(eng, "_xt", None) is not None:
        out += [host(t) for t in eng._xt]
    return out


def assert_x_untouched(eng, before):
    for a, b in zip(before, x_bytes(eng)):
        assert same(a, b), "the bit matrix was written to"


def xtu_slots_used(gpu, eng, blocked=False):
    """api.hip::xtu_slots_used: the slab slots the X^T U launch fills and the reduction sums"""
    L, E = gpu
    n = eng.splits_xtu
    if eng.panel == "i8":
        need = E.xf_slots_i8(eng.X.n_pad, eng.X.m_pad, 32 if blocked else eng.kp)
        n = min(n, need)
    return n


# ----------------------------------------------------------------------------------------------------------------------------------
# B. bmf_penalty_finalize on hand-made states
# ----------------------------------------------------------------------------------------------------------------------------------
_FIN = {}


def fin_engine(gpu, k):
    """an engine on the 40 x 30 dyadic case of rank k (kp = 32 at k = 5: one Gram entry per thread of finalize_kernel; kp = 64 at
    k = 33: four); nothing is prepared -- finalize_kernel reads comm, GV64, scal, stop, sum_x and cells only"""
    L, E = gpu
    if k not in _FIN:
        X, U, V = R.dyadic_case(k)
        eng = E.MUEngine(E.BitMatrix(X, DEV), k=k, mode=L.MODE_PENALTY, panel="bf16", terms=3, with_mae=True, tol=-1.0, min_diff=0.0, max_iter=20)
        assert eng.kp == (32 if k == 5 else 64) and eng.sum_x == float(X.sum()) and eng.log_rows == 22
        _FIN[k] = (eng, X, U, V, R.finalize_inputs(X, U, V, eng.kp))
    return _FIN[k]


def put_state(gpu, eng, inp, previous=MARK, stop=0, mode=None, with_mae=1, tol=-1.0, min_diff=0.0, max_iter=20):
    L, _ = gpu
    eng.comm.copy_(torch.from_numpy(inp["comm"]))
    eng.GV64.copy_(torch.from_numpy(inp["GV64"]))
    eng.scal.fill_(MARK)
    eng.scal[0] = inp["scal0"]
    eng.scal[1] = previous
    eng.GU.fill_(MARK)
    eng.log.fill_(MARK)
    eng.stop.fill_(stop)
    eng.st.mode = L.MODE_PENALTY if mode is None else mode
    eng.st.with_mae = with_mae
    eng.st.tol, eng.st.min_diff = tol, min_diff
    eng.max_iter = max_iter


def read_fin(eng):
    return snap(eng, ("log", "GU", "scal", "stop", "comm", "GV64"))


def assert_inputs_back(s, inp):
    assert same(s["comm"], inp["comm"]) and same(s["GV64"], inp["GV64"]) and s["scal"][0] == inp["scal0"]
    assert (s["scal"][2:] == MARK).all()


@pytest.mark.parametrize("k", [5, 33])
@pytest.mark.parametrize("mode,with_mae", [("penalty", 1), ("penalty", 0), ("wnmf", 1)])
def test_finalize_row_is_the_definition(gpu, k, mode, with_mae):
    """bmf_penalty_finalize -> finalize_kernel(do_gather = 0) -> finalize_body.  Every column of the row == driver_ref.log_row (the
    definition, from dense X, U, V); the inputs are dyadic, so no order of additions and no FMA can move a bit.  RMSE and MAE hold one
    fp64 divide and one square root of exact operands: gated at 1 ulp at first, they measured 0 ulp in all 24 cases on an MI355X (the
    device's fp64 divide and square root are correctly rounded) and are held to == since.  GU is the
    fp32 copy of comm[8..]; scal[1] is the watched value (reg_error in PENALTY mode, error in WNMF mode) after every call, iteration 0
    included; with_mae = 0 gives NaN; nothing else of the log, of scal or of the inputs moves."""
    L, _ = gpu
    eng, X, U, V, inp = fin_engine(gpu, k)
    md = L.MODE_PENALTY if mode == "penalty" else L.MODE_WNMF
    for it, reg in [(0, 0.5), (4, 3.25), (21, 2.0), (1, 0.0)]:
        put_state(gpu, eng, inp, mode=md, with_mae=with_mae, max_iter=50)
        eng.finalize(it, reg)
        s = read_fin(eng)
        want = R.log_row(X, U, V, it, reg, mode=md, with_mae=bool(with_mae))
        got = s["log"][it]
        for c in (R.ITER, R.ERROR, R.REC, R.REG, R.REGERR, R.TP, R.FP, R.FN, R.TN, R.VALID, R.STOP):
            assert got[c] == want[c] and np.signbit(got[c]) == np.signbit(want[c]), (it, c, got[c], want[c])
        print(f"k={k} {mode} it={it}: RMSE {ulps(got[R.RMSE], want[R.RMSE])} ulp" + (f", MAE {ulps(got[R.MAE], want[R.MAE])} ulp" if with_mae else ""))
        assert got[R.RMSE] == want[R.RMSE]
        if with_mae:
            assert got[R.MAE] == want[R.MAE]
        else:
            assert np.isnan(got[R.MAE])
        assert (got[13:] == MARK).all(), "spare columns written"
        others = np.delete(s["log"], it, axis=0)
        assert (others == MARK).all(), "another row written"
        assert same(s["GU"].ravel(), inp["comm"][8:].astype(np.float32))
        assert s["scal"][1] == R.watched(want, md) and s["stop"][0] == 0
        assert_inputs_back(s, inp)


def test_finalize_gu_rounds_to_nearest_even(gpu):
    """GU = float32(comm[8..]) in finalize_body: a tie (1 + 2^-24 -> 1), just above it (1 + 3 * 2^-25 -> 1 + 2^-23), values below the fp32
    normal range (kept as subnormals, rounded at 2^-149, ties to even), one that underflows to zero, signs kept."""
    L, _ = gpu
    eng, X, U, V, inp = fin_engine(gpu, 33)
    rs = np.random.RandomState(9)
    g = rs.randn(eng.kp * eng.kp) * 10.0 ** rs.randint(-30, 30, size=eng.kp * eng.kp)
    special = [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -25, -(1 + 2.0 ** -24), 1 + 2.0 ** -23 + 2.0 ** -24, 2.0 ** -130, 2.0 ** -130 + 2.0 ** -150,
               2.0 ** -130 + 3 * 2.0 ** -151, -(2.0 ** -140 + 2.0 ** -150), 2.0 ** -126 - 2.0 ** -160, 1e-50, -1e-50, 2.0 ** -150, 3 * 2.0 ** -151, 0.0, -0.0]
    g[:len(special)] = special
    g[-len(special):] = special          # (the last thread's entries too: i = tid + 3 * 1024)
    mine = dict(inp, comm=np.concatenate([inp["comm"][:8], g]))
    put_state(gpu, eng, mine)
    eng.finalize(2, 1.0)
    s = read_fin(eng)
    want = g.astype(np.float32)
    assert want[0] == 1.0 and want[1] == np.float32(1 + 2.0 ** -23) and want[3] == np.float32(1 + 2.0 ** -22) and want[5] == np.float32(2.0 ** -130)
    assert want[6] == np.float32(2.0 ** -130 + 2.0 ** -149) and want[9] == 0.0 and want[11] == 0.0 and want[12] == np.float32(2.0 ** -149)
    bad = np.flatnonzero(s["GU"].ravel().view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, [(int(i), float(g[i]), float(s["GU"].ravel()[i]), float(want[i])) for i in bad[:8]]
    assert_inputs_back(s, mine)


def test_finalize_negative_rec_gives_rmse_zero(gpu):
    """2 rec < 0 (comm[0] larger than any X allows): rec is logged as computed, RMSE is sqrt(max(2 rec, 0) / cells) = +0.0"""
    L, _ = gpu
    eng, X, U, V, inp = fin_engine(gpu, 5)
    comm = inp["comm"].copy()
    comm[0] = 2.0 ** 20
    mine = dict(inp, comm=comm)
    put_state(gpu, eng, mine)
    eng.finalize(3, 0.5)
    s = read_fin(eng)
    row = s["log"][3]
    b = float(np.dot(inp["comm"][8:], inp["GV64"]))
    assert row[R.REC] == 0.5 * (eng.sum_x - 2.0 * comm[0] + b) < 0
    assert row[R.RMSE] == 0.0 and not np.signbit(row[R.RMSE])
    assert_inputs_back(s, mine)


def _w(x):
    """a state whose watched value (PENALTY mode, reg = 1) is exactly x: reg * (0.5 * comm[1] + 0.5 * scal[0]) with comm[1] = 2 x, scal[0] = 0"""
    return {"comm1": 2.0 * x, "scal0": 0.0}


_UP = lambda x: float(np.nextafter(x, np.inf))     # noqa: E731
_DN = lambda x: float(np.nextafter(x, -np.inf))    # noqa: E731
# name: (iter, watched, previous, tol, min_diff, max_iter, stops)
STOP_EDGES = {
    "watched_equals_tol_stops": (1, 0.125, 9.0, 0.125, 0.0, 20, True),
    "watched_one_ulp_above_tol_goes_on": (1, _UP(0.125), 9.0, 0.125, 0.0, 20, False),
    "watched_one_ulp_below_tol_stops": (1, _DN(0.125), 9.0, 0.125, 0.0, 20, True),
    "diff_equals_min_diff_goes_on": (2, 0.0, 2.0, -1.0, 2.0, 20, False),
    "diff_one_ulp_below_min_diff_stops": (2, 0.0, _DN(2.0), -1.0, 2.0, 20, True),
    "diff_of_a_rising_value_counts_too": (2, 3.0, 1.0 + 2.0 ** -52, -1.0, 2.0, 20, True),
    "min_diff_zero_never_stops": (2, 1.0, 1.0, -1.0, 0.0, 20, False),
    "iter_equals_max_iter_goes_on": (7, 1.0, 9.0, -1.0, 0.0, 7, False),
    "iter_above_max_iter_stops": (8, 1.0, 9.0, -1.0, 0.0, 7, True),
    "iteration_zero_never_stops": (0, 0.0, 0.0, 1e9, 1e9, -1, False),
    "iteration_one_with_all_three_stops": (1, 0.0, 0.0, 1e9, 1e9, 0, True),
}


@pytest.mark.parametrize("name", list(STOP_EDGES))
def test_finalize_stop_rule_edges(gpu, name):
    """finalize_body's stopping rule against driver_ref.stop_rule (models/BaseModelTools.py:326-334): <= on tol, < on min_diff, > on
    max_iter, never at iteration 0.  Asserted: the flag (*stop == iter when it trips, 0 otherwise), row[LOG_STOP], scal[1]."""
    L, _ = gpu
    it, w, prev, tol, min_diff, max_iter, stops = STOP_EDGES[name]
    assert R.stop_rule(it, w, prev, tol, min_diff, max_iter) is stops
    eng, X, U, V, inp = fin_engine(gpu, 5)
    comm = inp["comm"].copy()
    comm[1] = 2.0 * w
    mine = dict(inp, comm=comm, scal0=0.0)
    put_state(gpu, eng, mine, previous=prev, tol=tol, min_diff=min_diff, max_iter=max_iter)
    eng.finalize(it, 1.0)
    s = read_fin(eng)
    row = s["log"][it]
    assert row[R.REGERR] == w and s["scal"][1] == w
    assert row[R.STOP] == float(stops) and s["stop"][0] == (it if stops else 0), (row[R.STOP], s["stop"])
    assert_inputs_back(s, mine)


def test_finalize_wnmf_watches_the_error(gpu):
    """mode PENALTY watches reg_error, mode WNMF the error (= rec_error): the same state, tol at one value or the other"""
    L, _ = gpu
    eng, X, U, V, inp = fin_engine(gpu, 5)
    rg = R.log_row(X, U, V, 1, 1.0)[R.REGERR]
    err = R.log_row(X, U, V, 1, 1.0, mode=R.MODE_WNMF)[R.ERROR]
    assert 0 < rg < err      # (U V^T of these factors is nowhere near X: the reconstruction error is the larger one)
    for md, tol, stops in ((L.MODE_PENALTY, rg, True), (L.MODE_PENALTY, _DN(rg), False), (L.MODE_WNMF, rg, False), (L.MODE_WNMF, err, True),
                           (L.MODE_WNMF, _DN(err), False)):
        put_state(gpu, eng, inp, previous=1e9, mode=md, tol=tol)
        eng.finalize(1, 1.0)
        s = read_fin(eng)
        assert s["stop"][0] == (1 if stops else 0) and s["log"][1, R.STOP] == float(stops), (md, tol, stops)
        assert s["scal"][1] == (rg if md == L.MODE_PENALTY else err)


def test_finalize_behind_a_raised_flag(gpu):
    """*stop = s already set.  finalize(iter > s) writes nothing: the marker survives in that row, GU, scal and stop are unchanged.
    finalize(iter <= s) is NOT a no-op -- it is the call that wrote row s in the first place, repeated: the row, GU and scal[1] are
    written again and the rule is evaluated again; the flag moves only when the rule trips (then to `iter`, which lowers it for
    iter < s) and is never cleared."""
    L, _ = gpu
    eng, X, U, V, inp = fin_engine(gpu, 5)
    for it in (4, 5, 21):
        put_state(gpu, eng, inp, stop=3, tol=1e9)
        eng.finalize(it, 1.0)
        s = read_fin(eng)
        assert (s["log"] == MARK).all() and (s["GU"] == MARK).all() and s["scal"][1] == MARK and s["stop"][0] == 3
        assert_inputs_back(s, inp)
    want = R.log_row(X, U, V, 3, 1.0)
    # iter == s, the rule does not trip now: row rewritten with LOG_STOP = 0, the flag stays
    put_state(gpu, eng, inp, stop=3)
    eng.finalize(3, 1.0)
    s = read_fin(eng)
    assert s["log"][3, R.REC] == want[R.REC] and s["log"][3, R.STOP] == 0.0 and s["stop"][0] == 3 and s["scal"][1] == want[R.REGERR]
    assert same(s["GU"].ravel(), inp["comm"][8:].astype(np.float32))
    # iter < s and the rule trips: the flag is lowered to iter; iter < s and it does not trip: the flag stays
    put_state(gpu, eng, inp, stop=3, tol=1e9)
    eng.finalize(2, 1.0)
    s = read_fin(eng)
    assert s["log"][2, R.STOP] == 1.0 and s["stop"][0] == 2 and s["log"][2, R.VALID] == 1.0
    put_state(gpu, eng, inp, stop=3)
    eng.finalize(2, 1.0)
    s = read_fin(eng)
    assert s["log"][2, R.STOP] == 0.0 and s["stop"][0] == 3 and s["log"][2, R.VALID] == 1.0


def test_finalize_refuses_rows_outside_the_log(gpu):
    L, _ = gpu
    eng, X, U, V, inp = fin_engine(gpu, 5)
    for it in (eng.log_rows, eng.log_rows + 5, -1):
        put_state(gpu, eng, inp, tol=1e9)
        with pytest.raises(L.BmfError):
            eng.finalize(it, 1.0)
        s = read_fin(eng)
        assert (s["log"] == MARK).all() and (s["GU"] == MARK).all() and s["scal"][1] == MARK and s["stop"][0] == 0
        assert_inputs_back(s, inp)


# ----------------------------------------------------------------------------------------------------------------------------------
# C. the slab sums
# ----------------------------------------------------------------------------------------------------------------------------------
def _nan_slabs(eng):
    eng.Nslab.fill_(float("nan"))
    eng._nred_flat.fill_(MARK)


def _check_slots(name, used):
    lo, hi = {"1-2": (1, 2), "5-7": (5, 7), "9+": (9, 10 ** 6), "any": (1, 10 ** 6)}[name]
    assert lo <= used <= hi, f"this device cuts X^T U into {used} slab slots; the case is named for {name}"


# (m, n, k, panel, slots): slot counts of the int8 plan on 256 compute units: 1, 1, 2 / 6, 6 / 10, 10; the bf16 / fp16 GEMM cuts by its own
# rule (whatever it gives is summed).  n_pad * kp is 32768 (reduce_slabs_kernel) at n = 500 and 65536 (reduce_slabs_wide_kernel) otherwise.
XTU_CASES = [(300, 500, 40, "i8", "1-2"), (300, 1000, 40, "i8", "1-2"), (700, 2048, 8, "i8", "1-2"),
             (3000, 500, 40, "i8", "5-7"), (3000, 1000, 40, "i8", "5-7"), (5000, 500, 40, "i8", "9+"), (5000, 1000, 40, "i8", "9+"),
             (300, 500, 40, "bf16", "any"), (300, 1000, 40, "bf16", "any"), (300, 500, 40, "f16", "any"), (300, 1000, 40, "f16", "any")]


@pytest.mark.parametrize("m,n,k,panel,slots", XTU_CASES)
def test_update_xtu_unblocked_sums_the_used_slots(gpu, m, n, k, panel, slots):
    """bmf_penalty_update_xtu(-1) -> sweep(SWEEP_XTU): the GEMM, then bmf_reduce_slabs over xtu_slots_used() slots -- reduce_slabs_kernel
    below n_pad * kp = 65536, reduce_slabs_wide_kernel from there on.  Nred == float32(fp64 sum of the device's own slabs in slot order).
    Every slot is pre-filled with NaN: the used ones must be rewritten in full, the others must stay NaN and never reach Nred."""
    eng = engine(gpu, m, n, k, panel)
    used = xtu_slots_used(gpu, eng)
    _check_slots(slots, used)
    wide = eng.X.n_pad * eng.kp >= 65536
    assert wide == (n != 500) and eng.Nslab.data_ptr() % 16 == 0 and eng._nred_flat.data_ptr() % 16 == 0 and eng.nred_blocks == 1
    before = snap(eng, FROZEN + DERIVED)
    xb = x_bytes(eng)
    _nan_slabs(eng)
    eng.local_xtu_block(-1)
    s = snap(eng, FROZEN + DERIVED + ("Nslab", "_nred_flat"))
    slabs = s["Nslab"]
    assert np.isfinite(slabs[:used]).all() and np.isnan(slabs[used:]).all()
    want = R.slab_sum_seq(slabs[:used]) if wide else R.slab_sum_grouped(slabs[:used])
    assert same(s["_nred_flat"], want.ravel())
    assert np.abs(want).max() > 0
    for name in FROZEN + DERIVED:     # X^T U writes the slabs and Nred, nothing else
        assert (before[name] is None and s[name] is None) or same(before[name], s[name]), name
    assert_x_untouched(eng, xb)


@pytest.mark.parametrize("m,n,k,slots", [(300, 1000, 40, "1-2"), (3000, 500, 40, "5-7"), (5000, 1000, 40, "9+")])
def test_update_xtu_blocked_sums_one_block_in_fp32(gpu, m, n, k, slots):
    """bmf_penalty_update_xtu(0), (1) with nred_blocks = 2 (int8 planes, kp = 64) -> reduce_slabs_block_kernel: block b of the block-major
    Nred [2][n_pad][32] == the fp32 slot-order sum of columns 32 b .. 32 b + 31 of the slabs; the other block is not touched.  Behind a
    raised flag the block is all +0.0 and the slabs are not touched."""
    eng = engine(gpu, m, n, k, "i8")
    assert eng.kp == 64 and eng.panel == "i8"
    eng.nred_blocks = eng.st.nred_blocks = 2
    used = xtu_slots_used(gpu, eng, blocked=True)
    _check_slots(slots, used)
    n_pad, half = eng.X.n_pad, eng.X.n_pad * 32
    xb = x_bytes(eng)
    before = snap(eng, FROZEN + DERIVED)
    _nan_slabs(eng)
    eng.local_xtu_block(0)
    s0 = snap(eng, ("Nslab", "_nred_flat"))
    assert np.isfinite(s0["Nslab"][:used, :, :32]).all() and np.isnan(s0["Nslab"][used:]).all()
    want0 = R.slab_sum_f32(s0["Nslab"][:used, :, :32])
    assert same(s0["_nred_flat"][:half].reshape(n_pad, 32), want0) and (s0["_nred_flat"][half:] == MARK).all()
    eng.local_xtu_block(1)
    s1 = snap(eng, FROZEN + DERIVED + ("Nslab", "_nred_flat"))
    assert np.isfinite(s1["Nslab"][:used, :, 32:]).all() and np.isnan(s1["Nslab"][used:]).all()
    want1 = R.slab_sum_f32(s1["Nslab"][:used, :, 32:])
    assert same(s1["_nred_flat"][half:].reshape(n_pad, 32), want1) and same(s1["_nred_flat"][:half], s0["_nred_flat"][:half])
    assert np.abs(want0).max() > 0 and np.abs(want1).max() > 0
    for name in FROZEN + DERIVED:
        assert (before[name] is None and s1[name] is None) or same(before[name], s1[name]), name
    # behind the flag
    _nan_slabs(eng)
    eng.stop.fill_(3)
    eng.local_xtu_block(1)
    s2 = snap(eng, ("Nslab", "_nred_flat", "stop"))
    assert np.isnan(s2["Nslab"]).all() and s2["stop"][0] == 3
    assert not s2["_nred_flat"][half:].view(np.uint32).any() and (s2["_nred_flat"][:half] == MARK).all()
    assert_x_untouched(eng, xb)


@pytest.mark.parametrize("m,n,k,panel,slots", [(300, 1000, 40, "i8", "1-2"), (700, 2048, 8, "i8", "1-2"), (3000, 1000, 40, "i8", "5-7"),
                                               (5000, 1000, 40, "i8", "9+"), (300, 1000, 40, "bf16", "any"), (700, 2048, 8, "f16", "any")])
def test_run_fused_reduction_sums_the_used_slots(gpu, m, n, k, panel, slots):
    """bmf_penalty_run of one iteration at a fused shape (n_pad * kp >= 65536, one block): the slab sum rides in reduce_finalize_kernel.
    Nred == the same fp64-then-round sum of the slabs read back; slots beyond xtu_slots_used() keep their NaN."""
    eng = engine(gpu, m, n, k, panel)
    used = xtu_slots_used(gpu, eng)
    _check_slots(slots, used)
    assert eng.nred_blocks == 1 and eng.X.n_pad * eng.kp >= 65536 and eng.Nslab.data_ptr() % 16 == 0 and eng._nred_flat.data_ptr() % 16 == 0
    xb = x_bytes(eng)
    eng.Nslab.fill_(float("nan"))      # (Nred is an input of this iteration's V update: it keeps the numerator of prepare())
    eng.run([1.5], it0=1)
    s = snap(eng, ("Nslab", "_nred_flat", "log", "stop"))
    assert s["stop"][0] == 0 and s["log"][1, R.VALID] == 1.0
    assert np.isfinite(s["Nslab"][:used]).all() and np.isnan(s["Nslab"][used:]).all()
    want = R.slab_sum_seq(s["Nslab"][:used])
    assert same(s["_nred_flat"], want.ravel()) and np.abs(want).max() > 0
    assert_x_untouched(eng, xb)


# ----------------------------------------------------------------------------------------------------------------------------------
# D. the gather
# ----------------------------------------------------------------------------------------------------------------------------------
def _full_count(eng):
    """(TP, FP) of the Boolean product of the device's own k-bit words against X, on the host"""
    X = data(eng.X.m, eng.X.n, eng.k)[0] != 0
    ub = host(eng.ubits)[: eng.X.m].view(np.uint64)
    vb = host(eng.vbits)[: eng.X.n].view(np.uint64)
    tp = fp = 0
    for r0 in range(0, eng.X.m, 4096):
        pd = (ub[r0:r0 + 4096, None] & vb[None, :]) != 0
        tp += int((pd & X[r0:r0 + 4096]).sum())
        fp += int((pd & ~X[r0:r0 + 4096]).sum())
    return tp, fp


@pytest.mark.parametrize("m,n,k", [(200, 150, 5), (33000, 100, 5)])
@pytest.mark.parametrize("form", ["update_head", "run"])
@pytest.mark.parametrize("delta", [True, False])
def test_gather_is_the_fixed_order_sum_of_the_partials(gpu, m, n, k, form, delta):
    """gather_kernel (after bmf_penalty_update_head) and gather_body inside the finalize launch (bmf_penalty_run): comm[0], comm[1],
    scal[0] == the sums of the epilogue partials read back, added as the kernel adds them (thread t takes blocks t, t + 256, ...; then
    the halving tree) -- at 33 000 rows there are 260 row blocks, so the strided loop runs twice.  counts[0:2] are reset; with the cover
    as running totals comm[2:4] == counts[2:4] == the full count; without, comm[2:4] == the full count and counts[2:4] are spare."""
    eng = engine(gpu, m, n, k, "i8", cover_delta=delta)
    assert eng.cover_delta == delta and (eng.X.m_pad // 128 > 256) == (m == 33000)
    xb = x_bytes(eng)
    eng.comm[:4] = MARK
    eng.scal[0] = MARK
    if not delta:
        eng.counts[2:] = 12345
    if form == "update_head":
        eng.local_update_head(1.5)
    else:
        eng.run([1.5], it0=1)
    s = snap(eng, ("comm", "scal", "counts", "partU", "partV", "stop", "log"))
    assert s["stop"][0] == 0
    dot, regu, regv = R.gather_sums(s["partU"], s["partV"])
    assert s["comm"][0] == dot and s["comm"][1] == regu and s["scal"][0] == regv and dot > 0 and regu > 0 and regv > 0
    assert (s["counts"][:2] == 0).all()
    tp, fp = _full_count(eng)
    assert tp > 0 and fp > 0
    assert s["comm"][2] == float(tp) and s["comm"][3] == float(fp)
    assert tuple(s["counts"][2:]) == ((tp, fp) if delta else (12345, 12345))
    if form == "run":
        assert s["log"][1, R.TP] == float(tp) and s["log"][1, R.FP] == float(fp) and s["log"][1, R.REGERR] == 1.5 * (0.5 * regu + 0.5 * regv)
    assert_x_untouched(eng, xb)


# ----------------------------------------------------------------------------------------------------------------------------------
# E. forms and the stop freeze
# ----------------------------------------------------------------------------------------------------------------------------------
FORMS = ("run", "phases", "update")


def iterate(eng, form, regs, it0=1):
    """iterations it0 .. through one of the three single-GPU forms of an iteration: (a) bmf_penalty_run; (b) bmf_penalty_update_head +
    _update_xtu(-1) + _finalize; (c) bmf_penalty_update + _finalize"""
    if form == "run":
        eng.run(regs, it0=it0)
        return
    for i, r in enumerate(regs):
        if form == "phases":
            eng.local_update_head(r)
            eng.local_xtu_block(-1)
        else:
            eng.local_update(r)
        eng.finalize(it0 + i, r)


def started(gpu, m, n, k, panel, regs0=1.0, **kw):
    eng = engine(gpu, m, n, k, panel, prepare=regs0, **kw)
    eng.log[1:] = MARK
    return eng


REGS6 = [1.0, 1.5, 2.25, 3.0, 4.5, 6.0]
SAME_IN_EVERY_FORM = FROZEN + DERIVED + ("_nred_flat",)


@pytest.mark.parametrize("panel", ["i8", "f16", "bf16"])
@pytest.mark.parametrize("m,n,k,presum", [(300, 500, 40, False), (300, 1000, 40, False), (700, 2048, 8, False), (300, 4000, 40, True),
                                          (3000, 1000, 40, False)])
def test_three_forms_give_the_same_bytes(gpu, panel, m, n, k, presum):
    """Six iterations through (a) bmf_penalty_run, (b) _update_head + _update_xtu(-1) + _finalize, (c) _update + _finalize, with the cover
    as running totals and as a full count, with both MAE passes and without.  Every form runs the same kernels on the same data in
    stream order -- the gather as a launch of its own or inside finalize, the slab sum of X^T U in reduce_slabs_[wide_]kernel or inside
    reduce_finalize_kernel (from n_pad * kp = 65536 on): the factors and shadows, bit words, panels and scales, Grams, the exchange
    block, Nred and every log row are byte-identical.  (300, 4000, 40): splits_xv >= 6, the in-place pre-sum of the X V slabs.
    (3000, 1000, 40): six X^T U slabs on int8 planes, so that the remainder loops of the two slab sums run.

    One exception, by design and written at bmf_penalty_state.stop: the exact-fp32 MAE pass (mae = 'f32': bmf_residual_sums) adds its
    workgroups' sums into comm[4], comm[5] with fp64 atomics, in the order the workgroups finish.  Those two and LOG_MAE = comm[4] /
    cells are then equal between two runs only up to the order of a sum of B non-negative numbers, B = the workgroups of
    bmf_residual_plan: each order is within gamma_(B-1) = (B - 1) u / (1 - (B - 1) u) of the exact sum relatively (u = 2^-53), two
    orders within 2 B u of each other, and the quotient adds a rounding each: 2 (B + 1) u.  (Seen at 3000 x 1000: last-place
    differences in comm[4], comm[5]; nothing else reads them.)  With the bf16 MAE pass (the default) or none, every byte agrees."""
    import ctypes as C
    L, _ = gpu
    g, per = C.c_int(0), C.c_int(0)
    assert L.lib.bmf_residual_plan(m, n, C.byref(g), C.byref(per)) == 0
    blocks, u = -(-m // 128) * g.value, 2.0 ** -53
    for delta in (True, False):
        for mae_kw in ({"with_mae": True, "mae": "bf16"}, {"with_mae": True, "mae": "f32"}, {"with_mae": False}):
            ref = None
            loose = {"comm": (slice(4, 6), 2 * blocks * u), "log": ((slice(None), R.MAE), 2 * (blocks + 1) * u)} if mae_kw.get("mae") == "f32" else {}
            for form in FORMS:
                eng = started(gpu, m, n, k, panel, cover_delta=delta, **mae_kw)
                if presum:
                    assert eng.splits_xv >= 6, eng.splits_xv
                elif panel == "i8":     # (the bf16 / fp16 GEMM cuts a short output finer: it pre-sums at the other shapes too)
                    assert eng.splits_xv < 6, eng.splits_xv
                fused = eng.X.n_pad * eng.kp >= 65536
                assert fused == (n != 500)
                if ref is None:
                    xb = x_bytes(eng)
                iterate(eng, form, REGS6)
                s = snap(eng, SAME_IN_EVERY_FORM)
                assert s["stop"][0] == 0 and (s["log"][:7, R.VALID] == 1.0).all() and (s["log"][7:] == MARK).all()
                assert np.isnan(s["log"][1:7, R.MAE]).all() == (not mae_kw["with_mae"])
                if ref is None:
                    ref = s
                    continue
                for name in SAME_IN_EVERY_FORM:
                    if ref[name] is None:
                        assert s[name] is None
                        continue
                    a, b = ref[name], s[name]
                    if name in loose:
                        where, rel = loose[name]
                        a, b = a.copy(), b.copy()
                        assert (np.abs(a[where] - b[where]) <= rel * np.maximum(np.abs(a[where]), np.abs(b[where]))).all(), (name, form, delta)
                        a[where] = b[where] = 0.0
                    assert same(a, b), (name, form, delta, mae_kw)
            assert_x_untouched(eng, xb)


def _trip(gpu, m, n, k, panel, trip):
    """(engine keywords, max_iter, regs, the iteration that trips): by tol at iteration 1, by min_diff at 2, by max_iter at 3"""
    regs = [4.0] * 8
    if trip == "tol":
        return {"tol": 1e30}, 12, regs, 1
    if trip == "max_iter":
        return {}, 2, regs, 3
    # min_diff: between the step of the watched value from iteration 1 to 2 and the (larger) one from 0 to 1 -- row 0 is written with
    # reg = 1, the others with reg = 4, so the first step is about three times the value itself
    eng = started(gpu, m, n, k, panel)
    eng.run(regs[:2], it0=1)
    w = snap(eng, ("log",))["log"][:3, R.REGERR]
    d1, d2 = abs(w[0] - w[1]), abs(w[1] - w[2])
    assert 0 < d2 < d1, (w, "the min_diff case needs a watched value that settles")
    return {"min_diff": 0.5 * (d1 + d2)}, 12, regs, 2


@pytest.mark.parametrize("trip", ["tol", "min_diff", "max_iter"])
@pytest.mark.parametrize("panel", ["i8", "f16", "bf16"])
@pytest.mark.parametrize("form", FORMS)
def test_stop_freezes_the_state(gpu, form, panel, trip):
    """Run A ends in the iteration that trips the rule, run B enqueues four more.  Every buffer of the state is then in one of three
    classes (the table at bmf_penalty_state.stop in include/bmf_hip.h):
      frozen   A == B by bytes: factors and shadows, bit words and previous words, cover totals, panels and scales, GU, GV, scal, the
               whole log (no row past the stop), stop;
      stated   comm[0..8): unchanged behind bmf_penalty_run (the gather rides in finalize, which returns at once), zeroed by
               gather_kernel in the stepwise forms; GV64 and comm[8..]: zeroed by the fused plane rebuild on int8 planes, rewritten to
               the same bytes from the unchanged factor on fp16 / bf16 panels; Nred in the stepwise forms: rewritten to the same bytes
               from the unchanged slabs (the blocked Nred, zeroed: test_update_xtu_blocked_sums_one_block_in_fp32);
      scratch  the slabs, panel_ws, partU / partV, mae_ws, and Nred behind bmf_penalty_run at this fused shape, whose slab sum races
               with the flag raised beside it: not compared."""
    m, n, k = 300, 1000, 40
    kw, max_iter, regs, s_it = _trip(gpu, m, n, k, panel, trip)
    out = []
    for extra in (0, 4):
        eng = started(gpu, m, n, k, panel, **kw)
        assert eng.X.n_pad * eng.kp >= 65536 and eng.nred_blocks == 1
        eng.max_iter = max_iter
        xb = x_bytes(eng)
        iterate(eng, form, regs[:s_it + extra])
        out.append(snap(eng, FROZEN + DERIVED + ("_nred_flat",)))
        assert_x_untouched(eng, xb)
    a, b = out
    assert a["stop"][0] == s_it and a["log"][s_it, R.STOP] == 1.0 and (a["log"][1:s_it, R.STOP] == 0.0).all()
    assert (a["log"][s_it + 1:] == MARK).all()
    for name in FROZEN:
        assert (a[name] is None and b[name] is None) or same(a[name], b[name]), (name, "moved behind the raised flag")
    kk = eng.kp * eng.kp
    assert a["comm"][0] > 0 and a["comm"][1] > 0 and np.abs(a["comm"][8:]).max() > 0 and np.abs(a["GV64"]).max() > 0
    if form == "run":
        assert same(a["comm"][:8], b["comm"][:8])
    else:
        assert not b["comm"][:8].view(np.uint64).any()
        assert same(a["_nred_flat"], b["_nred_flat"]) and np.abs(a["_nred_flat"]).max() > 0
    if panel == "i8":
        assert not b["comm"][8:].view(np.uint64).any() and not b["GV64"].view(np.uint64).any()
    else:
        assert same(a["comm"][8:], b["comm"][8:]) and same(a["GV64"], b["GV64"])
    assert b["comm"].size == 8 + kk
