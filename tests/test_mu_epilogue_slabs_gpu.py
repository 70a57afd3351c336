"""The numerator slabs of bmf_mu_epilogue with digit planes (csrc/epilogue.hip: mu_epilogue_i8_kernel<NT, MODE, LIMBS, S>): the forms with
a compile-time slab count (S = 1, 2, 3) keep every slab's raw value in the ring and add them when the chunk is consumed, the run-time
form (any other count) adds them as they are loaded.  Both must take the sum  ((+0 + s0) + s1) + ...  in fp32, in slab order.

The rule is stated here in NumPy float32 and handed to the kernel as ONE slab: a launch on S slabs and a launch with splits = 1 on
their sum must write the same bytes everywhere.  The slabs hold what makes a different sum visible: an all-zero slab (the GEMM's zero
fill), -0.0f entries (the sum starts from +0: an all -0.0f element gives +0), pairs that cancel exactly, and triples whose fp32 sum
depends on the order.  Two fp32 terms commute, so only three or more nonzero slabs can show a changed order: the host asserts that
every order a kernel could plausibly take instead (see other_orders) gives a different sum in some element; for two slabs it asserts
what can be seen there, that dropping either slab changes the sum.

Then the loop: three updates of MUEngine at the smallest shape of a short list whose X V launch really needs two slab slots, against
the fp64 oracle at the gates of tests/test_penalty_gpu.py.
"""
import numpy as np
import pytest

import oracle as orc
from test_mu_epilogue_cpu import PENALTY, WNMF, general_inputs
from test_mu_epilogue_gpu import launch

pytestmark = pytest.mark.gpu

ROWS_PAD, ROWS = 512, 390          # 128-row blocks: three full, one ragged (six valid rows) whose last three waves are all padding
OUTPUTS = ("F64", "F", "planes", "rowbits", "colbits", "partials", "blockmax")
# (slab count, what the slabs hold).  One slab cannot be all zero and carry a numerator, two cannot hold an all-zero slab and a pair,
# three cannot hold one and a triple: those counts run both ways.  From four on, slab 1 is all zero and the others hold everything.
SLAB_CASES = [(1, "single"), (2, "zero-slab"), (2, "pairs"), (3, "zero-slab"), (3, "triples"), (4, "all"), (7, "all")]


def sum32(slabs, order=None):
    """((+0 + s[order[0]]) + s[order[1]]) + ... in float32: the arithmetic rule, element by element"""
    acc = np.zeros(slabs.shape[1], np.float32)
    for j in (range(slabs.shape[0]) if order is None else order):
        acc = acc + slabs[j]
        assert acc.dtype == np.float32
    return acc


def other_orders(live):
    """Orders of the nonzero slabs `live` that a wrong kernel could take: reversed, every swap of two neighbours that is not the
    first two (those commute), and the last slab first."""
    out = [live[::-1], [live[-1]] + live[:-1]]
    for j in range(1, len(live) - 1):
        out.append(live[:j] + [live[j + 1], live[j]] + live[j + 2:])
    return out


def make_slabs(total, S, kind, rs):
    """S slabs [S][n] of float32 around the positive numerator `total` (flat), and the list of the slabs that are not all zero.
    Element e takes one of eight patterns (e % 8): 0-3 an ordinary split of mixed sign, 4 -0.0f in every slab, 5 a pair that cancels
    exactly (the rest -0.0f or +0), 6 the triple 2^24 t, t, -2^24 t with t a power of two (slab order gives 0: 2^24 t + t is a tie and
    goes to even; every other order gives t), 7 one -0.0f among ordinary terms."""
    n = total.size
    slabs = np.zeros((S, n), np.float32)
    zero = {"single": None, "zero-slab": 1, "pairs": None, "triples": None, "all": 1}[kind]
    live = [j for j in range(S) if j != zero]
    pat = np.arange(n) % 8
    c = rs.uniform(0.2, 1.0, (len(live), n)) / len(live)
    if len(live) >= 2:
        c[-1] *= -0.15                                  # mixed sign, the sum stays positive
    for i, j in enumerate(live):
        slabs[j] = (c[i] * total).astype(np.float32)
    slabs[:, pat == 4] = 0.0
    for j in live:
        slabs[j, pat == 4] = -0.0
    if len(live) >= 2:
        a, b = live[0], live[-1]
        x = slabs[a, pat == 5]
        slabs[:, pat == 5] = 0.0
        for j in live:
            slabs[j, pat == 5] = -0.0
        slabs[a, pat == 5], slabs[b, pat == 5] = x, -x
        slabs[live[len(live) // 2], pat == 7] = -0.0
    else:
        slabs[live[0], pat == 5] = 0.0
    if len(live) >= 3:
        t = np.exp2(np.floor(np.log2(total[pat == 6].astype(np.float64))) - 26).astype(np.float32)
        slabs[:, pat == 6] = 0.0
        slabs[live[0], pat == 6], slabs[live[1], pat == 6], slabs[live[2], pat == 6] = t * np.float32(2.0 ** 24), t, -t * np.float32(2.0 ** 24)
    return slabs, live


@pytest.mark.parametrize("S,kind", SLAB_CASES, ids=["%d-%s" % c for c in SLAB_CASES])
@pytest.mark.parametrize("limbs", [2, 3])
@pytest.mark.parametrize("mode", [PENALTY, WNMF], ids=["penalty", "wnmf"])
@pytest.mark.parametrize("k,kp", [(20, 32), (40, 64)])
def test_slabs_are_added_in_order_from_plus_zero(k, kp, mode, limbs, S, kind):
    c = dict(form="planes%d" % limbs, mode=mode, k=k, kp=kp, rows_pad=ROWS_PAD, rows=ROWS, layout="plain", splits=1,
             reg=1.5 if mode == PENALTY else 2.5, seed=6100 + 8 * S + limbs + kp)
    a = general_inputs(c)
    n = ROWS_PAD * kp
    stride = a["slab_stride"]
    assert stride > n and a["num_block_stride"] == 0
    rs = np.random.RandomState(c["seed"] + 1)
    slabs, live = make_slabs(a["num"][0, :n].copy(), S, kind, rs)
    want = sum32(slabs)
    check_inputs(slabs, live, want, kind)

    # ---- the launch on S slabs against the launch on their sum ----
    def with_num(rows_of_num):
        num = np.full((rows_of_num.shape[0], stride), 3.0, np.float32)          # junk between and behind the slabs
        num[:, :n] = rows_of_num
        return dict(a, num=num, splits=rows_of_num.shape[0])

    got = launch(with_num(slabs))
    ref = launch(with_num(want[None, :]))
    assert set(got) == set(ref) == set(OUTPUTS)
    for name in OUTPUTS:
        differ = np.argwhere(got[name].view(np.uint8) != ref[name].view(np.uint8))[:4].tolist()
        assert got[name].tobytes() == ref[name].tobytes(), f"{name}: {len(differ)}+ bytes differ, first at {differ}"
    # the step did something: the numerator reaches the new factor and the second partial
    ok = (np.arange(ROWS_PAD)[:, None] < ROWS) & (np.arange(kp)[None, :] < k)
    assert (got["F64"][ok] != a["F64"][ok]).mean() > 0.9 and (got["partials"][:, 1] != 0).all()


def check_inputs(slabs, live, want, kind):
    """the inputs can show what they are there to show (host only)"""
    S, n = slabs.shape
    signbit = np.signbit(slabs)
    assert (slabs == 0).all(axis=1).sum() == S - len(live)                       # the all-zero slab, +0 throughout
    assert not signbit[[j for j in range(S) if j not in live]].any()
    assert (signbit & (slabs == 0)).any()                                        # -0.0f entries ...
    allneg0 = (signbit & (slabs == 0))[live].all(axis=0)
    assert allneg0.any() and not np.signbit(want[allneg0]).any() and not want[allneg0].any()   # ... whose sum from +0 is +0
    if len(live) >= 2:
        cancel = (slabs[live[0]] == -slabs[live[-1]]) & (slabs[live[0]] != 0)
        assert cancel.sum() > n // 16 and not want[cancel].any()                 # pairs that cancel exactly
        for j in live:                                                           # no slab can be dropped unseen
            assert (sum32(slabs, [i for i in range(S) if i != j]) != want).any()
    if len(live) >= 3:
        for order in other_orders(live):                                         # no other order goes unseen
            differs = sum32(slabs, order) != want
            assert differs.sum() > n // 64, (order, differs.sum())
        # (nor the other rule the library has for slabs: fp64 sum, one rounding -- bmf_reduce_slabs)
        assert (slabs.astype(np.float64).sum(axis=0).astype(np.float32) != want).any()
    elif S == 2 and kind == "pairs":
        # two terms commute in fp32: a swapped order cannot change a two-slab sum, only a third term can
        assert np.array_equal(sum32(slabs, [1, 0]).view(np.uint32), want.view(np.uint32))


# ---- the loop at a shape whose X V launch writes two slabs -----------------------------------------------------------------------------
LOOP_SHAPES = [(2048, 1536), (4096, 2048), (8192, 4096)]
FACTOR_TOL = 1e-4      # tests/test_penalty_gpu.py
SCALAR_TOL = 1e-4


def test_three_updates_at_a_shape_with_two_slabs():
    from pybmf_amd import _lib as L
    from pybmf_amd.engine import BitMatrix, MUEngine, round_up, xf_slots_i8
    k, kp = 40, 64
    found = None
    for m, n in LOOP_SHAPES:
        slots = xf_slots_i8(round_up(m, L.ROW_PAD), round_up(n, L.ROW_PAD), kp)
        print(f"{m} x {n}: X V needs {slots} slab slot(s)")
        if slots >= 2 and found is None:
            found = (m, n, slots)
    assert found is not None, "no shape of the list needs two slab slots for X V"
    m, n, slots = found
    X, _, _, _ = orc.synthetic_boolean(m, n, k, (0.1, 0.1), seed=21)
    X = orc.flip_noise(X, (0.05, 0.01), seed=22)
    ref = orc.penalty_fit(X, k=k, reg=1.0, reg_growth=1.05, init_method="normal", normalize_method="balance", max_iter=2, seed=4, literal=False)
    eng = MUEngine(BitMatrix(X.astype(np.uint8), "cuda:0"), k=k, mode=L.MODE_PENALTY, panel="i8", terms=3, with_mae=True, max_iter=2)
    assert eng.splits_xv == slots and eng.kp == kp
    eng.load_factors(orc.zeros_to_eps(ref["U0"]), orc.zeros_to_eps(ref["V0"]))
    regs = [1.0 * 1.05 ** i for i in range(3)]
    eng.prepare(regs[0])
    eng.run(regs, it0=1)
    log, stop = eng.read_log()
    U, V = eng.factors()
    want = np.array(ref["updates"])
    assert want.shape[0] == 4                                                   # the initial row and three updates
    got = log[:, [L.LOG_ITER, L.LOG_ERROR, L.LOG_REC, L.LOG_REG, L.LOG_REGERR, L.LOG_RMSE, L.LOG_MAE]]
    assert got.shape == want.shape, (got.shape, want.shape)
    relf = lambda x, y: np.linalg.norm(x - y) / np.linalg.norm(y)   # noqa: E731
    print(f"scalars: worst relative difference {np.abs(got[:, 1:] / want[:, 1:] - 1).max():.2e}; U {relf(U, ref['U']):.2e}  V {relf(V, ref['V']):.2e}")
    np.testing.assert_allclose(got, want, rtol=SCALAR_TOL)
    assert relf(U, ref["U"]) < FACTOR_TOL and relf(V, ref["V"]) < FACTOR_TOL
