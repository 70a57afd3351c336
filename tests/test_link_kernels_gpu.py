"""Every kernel of the dense link family (csrc/link.hip) by direct C ABI calls, element by element against the fp64 restatements of
tests/link_ref.py (pinned to the oracle by tests/test_link_kernels_cpu.py), evaluated on the fp32-rounded factors the kernels see.

Which instantiation and which pipeline length each case of R.PASS_CASES reaches (tiles = 32-column tiles per workgroup; the pipelined
link_pass16sp_kernel<KP, LINK> runs prologue + (tiles - 1) loop trips + epilogue over a ring of three LDS buffers; every case runs both
links and both kp come from the k cycle 5 / 32 / 40 / 64):

  rows x cols (X orientation)                          row blocks  slabs x tiles            what it is there for
  {1, 32, 33, 128, 129} x 1                            1 / 2       1 x 1                    no loop trip, fetch(min(1, ntile - 1)) clamped
  ... x 33                                             1 / 2       1 x 2                    one loop trip
  ... x 65                                             1 / 2       1 x 3                    every ring buffer once
  ... x 97                                             1 / 2       1 x 4                    first wrap of the ring
  ... x 129, ... x 193                                 1 / 2       1 x 5, 1 x 7             further wraps
  33 x 16, 129 x 49, 32 x 63, 128 x 64                 1 / 2       1 x 1, 1 x 2             16, 17, 31, 32 valid columns in the last tile
  130 x 545                                            2           2 x 9                    two equal slabs
  130 x 515                                            2           9 + 8                    a shorter second slab
  130 x 4100                                           2           14 x 9 + 3               many slabs, a short last one
  the same cases transposed (X^T, V, U)                1 .. 33     1 x {1, 2, 4, 5}         many row blocks; the other orientation
  rows 1 / 32 / 33 / 128 / 129                         the last valid row at position 0 / 31 / 32 / 127 of its block / 0 of a second block
  localisation: 1024 x 128, 1024 x 224                 8           1 x 4, 1 x 7             one cell per row, every in-tile position

  link_pass_kernel<KP, LINK>, link_sums_kernel<KP, LINK>, link_sums16_kernel<KP, LINK> (interior / edge cell loops: the edge form for the
  last row block and the last column tile, the interior form for every other tile, e.g. rows 128 / 129 x cols 65 .. 193) run at the same
  cases.  link_pass_kernel<KP, SIGMOID> forms P from KP / 2 MFMA steps added in fp64, <KP, KL> in one fp32 accumulator.

Gates.  fp32 kernels: rtol 2e-5 + atol 1e-6 on num / den, 2e-5 relative on the sums (the gates of tests/test_link_gpu.py).  16-bit pass and
sums: the element-wise bounds R.pass16_bound / R.sums16_bound, every term named there, no fitted constant.  Split workspaces: bit for bit.
Column sums: exact on integers, else half an fp32 ulp + rows 2^-53 sum |v|.  No entry is left out of any comparison.  Every case records
its worst error as a fraction of its gate; run with -s to see the table printed when the module ends."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import link_ref as R  # noqa: E402

WORST = {}
LINKS = [(R.LINK_SIGMOID, 1.0), (R.LINK_SIGMOID, 10.0), (R.LINK_SIGMOID, 300.0), (R.LINK_KL, 1.0)]
LINK_NAME = {R.LINK_SIGMOID: "sigmoid", R.LINK_KL: "kl"}
SENTINEL = -7.0


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield
    print()
    for key in sorted(WORST, key=str):
        print("WORST", key, " ".join(f"{n}={v:.3g}" for n, v in sorted(WORST[key].items())))


def note(key, **figures):
    slot = WORST.setdefault(key, {})
    for name, value in figures.items():
        slot[name] = max(slot.get(name, 0.0), float(value))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    a = np.array(a, order="C")               # a copy: the shared host inputs are read-only
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def off(t, nbytes):
    """device pointer of tensor t moved by nbytes (for the alignment refusals)"""
    return C.c_void_p(t.data_ptr() + nbytes)


def last_error():
    from pybmf_amd import _lib as L
    msg = L.lib.bmf_last_error()
    return msg.decode() if msg else ""


# ---------------------------------------------------------------------------------------------------------------------------------------
# device forms of the shared cases
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_bits(rows, cols, poison=False):
    """X and X^T as bit words on the device, each with one word of ones past the last column tile in every row"""
    X = R.make_X(rows, cols)
    ldx, ldxt = (cols + 31) // 32 + 1, (rows + 31) // 32 + 1
    return dev(R.pack_bits(X, R.pad128(rows), ldx, poison)), dev(R.pack_bits(X.T, R.pad128(cols), ldxt, poison)), ldx, ldxt


def new_ws(rows_pad, kp):
    return torch.full((5 * rows_pad * kp,), 0x5A5A, dtype=torch.int16, device="cuda")


@functools.lru_cache(maxsize=6)
def case_factors(rows, cols, k, name, poison=False):
    """the factors of a case zero padded to (pad128, kp) on the device, and their bmf_link_split_pair workspaces"""
    from pybmf_amd import _lib as L
    U, V = R.make_factors(rows, cols, k, name)
    kp, m_pad, n_pad = R.kp_of(k), R.pad128(rows), R.pad128(cols)
    Ud = dev(R.padded_factor(U, m_pad, kp, R.poison_row(U) if poison else None))
    Vd = dev(R.padded_factor(V, n_pad, kp, R.poison_row(V) if poison else None))
    wsU, wsV = new_ws(m_pad, kp), new_ws(n_pad, kp)
    L.check(L.lib.bmf_link_split_pair(L.ptr(Ud), m_pad, L.ptr(Vd), n_pad, kp, L.ptr(wsU), L.ptr(wsV), stream()), "bmf_link_split_pair")
    return dict(U=U.astype(np.float64), V=V.astype(np.float64), Ud=Ud, Vd=Vd, wsU=wsU, wsV=wsV, kp=kp, m_pad=m_pad, n_pad=n_pad)


def oriented(rows, cols, k, name, transposed, poison=False):
    """one orientation of a case: (X, F_self, F_other on the host; bits, ldx, rows, cols, pads, device factors and workspaces)"""
    bits, bits_t, ldx, ldxt = case_bits(rows, cols, poison)
    f = case_factors(rows, cols, k, name, poison)
    X = R.make_X(rows, cols)
    if transposed:
        return dict(X=X.T, Fs=f["V"], Fo=f["U"], bits=bits_t, ldx=ldxt, rows=cols, cols=rows, rows_pad=f["n_pad"], other_pad=f["m_pad"],
                    Fsd=f["Vd"], Fod=f["Ud"], ws_s=f["wsV"], ws_o=f["wsU"], kp=f["kp"], k=k)
    return dict(X=X, Fs=f["U"], Fo=f["V"], bits=bits, ldx=ldx, rows=rows, cols=cols, rows_pad=f["m_pad"], other_pad=f["n_pad"],
                Fsd=f["Ud"], Fod=f["Vd"], ws_s=f["wsU"], ws_o=f["wsV"], kp=f["kp"], k=k)


def run_pass(o, kind, link, lam, over=None):
    """one call of bmf_link_pass (kind 'f32') or bmf_link_pass16 ('16'); returns (rc, num slabs, den slabs) as host arrays.  `over`
    replaces arguments for the refusal tests."""
    from pybmf_amd import _lib as L
    splits = L.lib.bmf_link_splits(o["rows"], o["cols"])
    assert splits == R.splits_for(o["rows"], o["cols"])
    stride = o["rows_pad"] * o["kp"]
    num = torch.full((splits + 1, o["rows_pad"], o["kp"]), SENTINEL, device="cuda")
    den = torch.full((splits + 1, o["rows_pad"], o["kp"]), SENTINEL, device="cuda")
    a = dict(self=L.ptr(o["Fsd"] if kind == "f32" else o["ws_s"]), other=L.ptr(o["Fod"] if kind == "f32" else o["ws_o"]), link=link,
             den=L.ptr(den), stride=stride, splits=splits)
    a.update(over or {})
    fn = L.lib.bmf_link_pass if kind == "f32" else L.lib.bmf_link_pass16
    rc = fn(L.ptr(o["bits"]), o["rows_pad"], o["ldx"], o["rows"], o["cols"], a["self"], a["other"], o["other_pad"], o["kp"], a["link"],
            float(lam), L.ptr(num), a["den"], a["stride"], a["splits"], stream())
    return rc, num.cpu().numpy(), den.cpu().numpy()


def slab_sum(slabs, splits):
    acc = np.zeros(slabs.shape[1:], np.float64)
    for s in range(splits):                    # in slab order, fp64
        acc += slabs[s].astype(np.float64)
    return acc


@functools.lru_cache(maxsize=4)
def wanted(rows, cols, k, name, link, lam, transposed):
    o = oriented(rows, cols, k, name, transposed)
    num, den = R.pass_ref(o["X"], o["Fs"], o["Fo"], link, lam)
    gnum, gden = R.pass16_bound(o["X"], o["Fs"], o["Fo"], link, lam, R.pass_acc(o["cols"]))
    return num, den, gnum, gden


def fraction(err, gate):
    """max err / gate; an entry whose gate is 0 must be exact"""
    assert (err[gate == 0] == 0).all()
    live = gate > 0
    return float((err[live] / gate[live]).max()) if live.any() else 0.0


def check_pass(o, kind, link, lam, got, want, key):
    rc, num, den = got
    wnum, wden, gnum, gden = want
    rows, k, X = o["rows"], o["k"], o["X"]
    splits = R.splits_for(rows, o["cols"])
    assert rc == 0, last_error()
    assert (num[splits] == SENTINEL).all() and (den[splits] == SENTINEL).all()          # nothing past the last slab
    assert np.isfinite(num[:splits]).all() and (num[:splits] >= 0).all()                 # every entry of every slab overwritten
    assert (num[:splits, rows:] == 0).all() and (num[:splits, :, k:] == 0).all()         # padded rows and padded kp columns: exactly 0
    assert (num[:splits, :rows][:, X.sum(axis=1) == 0] == 0).all()                       # rows whose X row is empty: exactly 0
    n = slab_sum(num, splits)[:rows, :k]
    if link == R.LINK_SIGMOID:
        assert np.isfinite(den[:splits]).all() and (den[:splits] >= 0).all() and (den[:splits, :, k:] == 0).all()
        d = slab_sum(den, splits)[:rows, :k]
    else:
        assert (den == SENTINEL).all()                                                   # KL: den is not written
    if kind == "f32":
        fn = fraction(np.abs(n - wnum), R.FP32_ATOL + R.FP32_RTOL * np.abs(wnum))
        fd = fraction(np.abs(d - wden), R.FP32_ATOL + R.FP32_RTOL * np.abs(wden)) if link == R.LINK_SIGMOID else 0.0
    else:
        fn = fraction(np.abs(n - wnum), gnum)
        fd = fraction(np.abs(d - wden), gden) if link == R.LINK_SIGMOID else 0.0
        live = np.abs(wnum) > gnum               # entries above their own gate: where the clamp floor is not the whole of it
        note(key, num_gate_live=fraction(np.abs(n - wnum)[live], gnum[live]))
    note(key, num_gate=fn, den_gate=fd)
    assert fn <= 1.0 and fd <= 1.0, (key, o["rows"], o["cols"], k, fn, fd)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. bmf_link_pass and bmf_link_pass16
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,k", R.PASS_CASES)
def test_pass_element_by_element(rows, cols, k):
    """Both pass kernels at every case of the table: four factor sets (the saturating one for the sigmoid link only: it is defined by
    lam), both links, lam 1 / 10 / 300, both orientations; num and den element-wise over every valid entry after summing the slabs in
    slab order, exact zeros where the contract says so.  The KL pass ignores lam (bit-identical at lam = 300).

    Measured on an MI355X, worst fraction of the gate over all 37 cases and both orientations (num | den):
      bmf_link_pass16, derived bound    sigmoid lam 1: 0.44 | 0.47   lam 10: 0.38 | 0.36   lam 300: 0.41 | 0.16 (entries above their own
                                        gate; the entries that are nothing but the 2^-100 clamp meet their floor at 1.00 by construction)
                                        KL: 0.47 (moderate 0.46, unbalanced 0.47, zero rows 0.29)
      bmf_link_pass, rtol 2e-5 + 1e-6   sigmoid lam 1: 0.04 | 0.05   lam 10: 0.05 | 0.05   lam 300: 0.38 | 0.59   KL: 0.024
    Two terms of the derived bound were corrected after the first run, the derivation and not the kernel being short both times (see
    R.PROD and the floor in R.pass16_bound): a contraction product is right to 3 x 2^-16, not 2^-16 (the single-term KL rows of the
    97 x 1 case came out at 1.4 x 2^-16), and the clamp floor carries the relative terms of a live cell.
    The fp32 pass at lam = 300 was a defect this test found: with P accumulated in fp32 it missed its gate in 41 of 296 runs (worst 3.07 |
    3.59 of it, saturating set, 4100 x 130, k = 64), because s = lam (P - 1/2) multiplies the 2 - 4 ulp that the accumulation leaves on a
    P near 1/2 by 300.  link_pass_kernel now adds the MFMA steps of P in fp64 for the sigmoid link; the figures above are after that."""
    for name in R.FACTOR_SETS:
        for link, lam in LINKS:
            if link == R.LINK_KL and name == "saturating":
                continue
            for transposed in (False, True):
                o = oriented(rows, cols, k, name, transposed)
                want = wanted(rows, cols, k, name, link, lam, transposed)
                for kind in ("f32", "16"):
                    got = run_pass(o, kind, link, lam)
                    check_pass(o, kind, link, lam, got, want, ("pass" + kind, LINK_NAME[link], name, f"lam{lam:g}"))
                    if link == R.LINK_KL and name == "moderate":
                        again = run_pass(o, kind, link, 300.0)
                        assert np.array_equal(got[1], again[1])


@pytest.mark.parametrize("rows,cols,k", [(33, 65, 5), (129, 193, 32), (128, 97, 40), (130, 515, 40), (33, 16, 32)])
def test_fp32_pass_ignores_finite_poison_in_every_padding(rows, cols, k):
    """bmf_link_pass masks by row_ok and the column bound: ones in the padding bits of X (last tile and padding rows) and finite values in
    the padding rows of both factors change nothing, bit for bit.  (bmf_link_pass16 has no such mask: its contract is zero padding.)"""
    for name, link, lam in (("moderate", R.LINK_SIGMOID, 10.0), ("saturating", R.LINK_SIGMOID, 300.0), ("zero_rows", R.LINK_KL, 1.0)):
        for transposed in (False, True):
            clean = run_pass(oriented(rows, cols, k, name, transposed), "f32", link, lam)
            dirty = run_pass(oriented(rows, cols, k, name, transposed, poison=True), "f32", link, lam)
            assert clean[0] == 0 and dirty[0] == 0
            assert np.array_equal(clean[1], dirty[1]) and np.array_equal(clean[2], dirty[2])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. cell localisation
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", R.LOCAL_TILES)
@pytest.mark.parametrize("k", [32, 64])
def test_pass_puts_every_cell_where_it_belongs(k, tiles):
    """Row i of X has its single one at column pi(i); over the 1024 rows every (row, column) position of the 32 x 32 tile and every tile
    index of the sweep is hit.  num[i, :] must be g(i, pi(i)) F_other[pi(i), :] -- one term, no accumulation: a wrong row mapping, a wrong
    4 h shift, an X word taken from the neighbouring tile or a ring buffer read one tile late all put another row of F_other there."""
    from pybmf_amd import _lib as L
    rows, cols, kp = R.LOCAL_ROWS, 32 * tiles, k
    pi = R.local_pi(tiles)
    X = np.zeros((rows, cols), np.uint8)
    X[np.arange(rows), pi] = 1
    U, V = R.make_factors(rows, cols, k, "moderate")
    Ud, Vd = dev(U), dev(R.padded_factor(V, R.pad128(cols), kp))
    wsU, wsV = new_ws(rows, kp), new_ws(R.pad128(cols), kp)
    L.check(L.lib.bmf_link_split_pair(L.ptr(Ud), rows, L.ptr(Vd), R.pad128(cols), kp, L.ptr(wsU), L.ptr(wsV), stream()))
    o = dict(X=X, Fs=U.astype(np.float64), Fo=V.astype(np.float64), bits=dev(R.pack_bits(X, rows, tiles + 1)), ldx=tiles + 1, rows=rows, cols=cols,
             rows_pad=rows, other_pad=R.pad128(cols), Fsd=Ud, Fod=Vd, ws_s=wsU, ws_o=wsV, kp=kp, k=k)
    for link, lam in ((R.LINK_SIGMOID, 10.0), (R.LINK_KL, 1.0)):
        _, _, g1, _ = R.link_cells(X, o["Fs"], o["Fo"], link, lam)
        want = g1[np.arange(rows), pi][:, None] * o["Fo"][pi]                     # the single term, written out
        num, den = R.pass_ref(X, o["Fs"], o["Fo"], link, lam)
        np.testing.assert_allclose(num, want, rtol=1e-14, atol=0)
        gnum, gden = R.pass16_bound(X, o["Fs"], o["Fo"], link, lam, 0)            # the single-product bound: no accumulation term
        for kind in ("f32", "16"):
            check_pass(o, kind, link, lam, run_pass(o, kind, link, lam), (want, den, gnum, gden), ("local" + kind, LINK_NAME[link], f"kp{kp}"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. bmf_link_sums and bmf_link_sums16
# ---------------------------------------------------------------------------------------------------------------------------------------
PRESET = np.array([3.5, -2.25, 7.125, 11.0])


def run_sums(f, bits, ldx, rows, cols, kind, link, lam, obits):
    from pybmf_amd import _lib as L
    sums = dev(PRESET.copy())
    a, b = (f["Ud"], f["Vd"]) if kind == "f32" else (f["wsU"], f["wsV"])
    fn = L.lib.bmf_link_sums if kind == "f32" else L.lib.bmf_link_sums16
    L.check(fn(L.ptr(bits), f["m_pad"], ldx, rows, cols, L.ptr(a), L.ptr(b), f["n_pad"], f["kp"], link, float(lam), L.ptr(obits), L.ptr(sums),
               stream()), "bmf_link_sums" + ("" if kind == "f32" else "16"))
    got = sums.cpu().numpy()
    assert got[3] == PRESET[3]                                                   # three words are the kernel's, the fourth is not
    return got[:3] - PRESET[:3]                                                  # the kernels ADD to what the words hold


@pytest.mark.parametrize("rows,cols,k", R.PASS_CASES)
def test_sums_against_every_cell(rows, cols, k):
    """Both sums kernels at every case: Obits null / a random pattern / empty; sums[0] and sums[1] do not depend on it, sums[2] is restricted
    to it; accumulators preset to non-zero values; and the same with ones in every padding bit of X and Obits and finite values in the
    padding rows of the factors (masked by row_ok and the column bound: unchanged).

    Measured on an MI355X, worst fraction of the gate (sums[0] | sums[1] | sums[2]):
      bmf_link_sums16, derived bound   sigmoid 0.080 | 0.086 | -     KL 0.044 | 0.057 | 0.027
      bmf_link_sums, 2e-5 relative     sigmoid 0.20 | 0.39 | - (lam 300, saturating; 0.04 | 0.08 at lam 10)     KL 0.005 | 0.009 | 0.012"""
    X = R.make_X(rows, cols)
    rs = np.random.RandomState(rows + 3 * cols)
    O = (rs.rand(rows, cols) < 0.6).astype(np.uint8)
    O[rows - 1, cols - 1], O[0, 0] = 1, 1                                        # the corner cell and the zero-row cell are observed
    m_pad, ldx = R.pad128(rows), (cols + 31) // 32 + 1
    patterns = {"null": None, "random": O, "empty": np.zeros_like(O)}
    for name, link, lam in (("moderate", R.LINK_SIGMOID, 10.0), ("saturating", R.LINK_SIGMOID, 300.0), ("moderate", R.LINK_KL, 1.0),
                            ("zero_rows", R.LINK_KL, 1.0)):
        f = case_factors(rows, cols, k, name)
        fp = case_factors(rows, cols, k, name, True)
        bits, bits_p = case_bits(rows, cols)[0], case_bits(rows, cols, True)[0]
        wants = {oname: R.sums_ref(X, f["U"], f["V"], link, lam, Oh) for oname, Oh in patterns.items()}
        bounds = {oname: R.sums16_bound(X, f["U"], f["V"], link, lam, Oh) for oname, Oh in patterns.items()}
        for kind in ("f32", "16"):
            seen = {}
            for oname, Oh in patterns.items():
                want = wants[oname]
                got = run_sums(f, bits, ldx, rows, cols, kind, link, lam, None if Oh is None else dev(R.pack_bits(Oh, m_pad, ldx)))
                err = np.abs(got - want)
                gate = 2e-5 * np.abs(want) if kind == "f32" else bounds[oname]
                gate = gate + 2.0 ** -50 * np.abs(PRESET[:3])                    # taking the preset off again rounds in fp64
                key = ("sums" + kind, LINK_NAME[link], name)
                note(key, **{f"s{q}_gate": err[q] / gate[q] for q in range(3) if want[q] != 0})
                assert (err <= gate).all(), (key, oname, got, want, err / gate)
                if link == R.LINK_SIGMOID or Oh is not None and not Oh.any():
                    assert got[2] == 0.0                                         # nothing observed, or no KL term: exactly nothing added
                seen[oname] = got
                dirty = run_sums(fp, bits_p, ldx, rows, cols, kind, link, lam, None if Oh is None else dev(R.pack_bits(Oh, m_pad, ldx, True)))
                np.testing.assert_allclose(dirty, got, rtol=1e-12, atol=2.0 ** -50 * 11)
            for oname in ("random", "empty"):                                    # the pattern restricts sums[2] only
                np.testing.assert_allclose(seen[oname][:2], seen["null"][:2], rtol=1e-12, atol=2.0 ** -50 * 11)
            if wants["random"][2] != wants["null"][2]:
                assert seen["random"][2] != seen["null"][2]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. bmf_link_split and bmf_link_split_pair
# ---------------------------------------------------------------------------------------------------------------------------------------
def same_words(got, want, what, lo=None):
    """bit-for-bit equality; on a mismatch says how many of the differing words sit where the fp16 lo addend is subnormal"""
    bad = got != want
    if bad.any():
        where = ""
        if lo is not None:
            v = np.abs(lo.view(np.float16).astype(np.float64))
            where = f", {int((bad & (v < 2.0 ** -14)).sum())} of them where the expected lo is subnormal or zero"
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ{where}; first at {i}: got {int(got[i]):#06x}, want {int(want[i]):#06x}")


def ws_arrays(ws, n):
    w = ws.cpu().numpy().view(np.uint16)
    return [w[i * n:(i + 1) * n] for i in range(5)]


def check_ws(ws, F, kp, scale, head, what):
    n = F.size
    hi, lo, third, ph, pl = ws_arrays(ws, n)
    want = R.split_words(F, scale)
    words = third.view(np.uint32)
    assert np.array_equal(words[:head.size], head), (what, "header", words[:head.size], head)
    assert (third[2 * head.size:] == 0x5A5A).all(), what + ": the rest of the third array is not the split's to write"
    same_words(hi, want["hi"], what + " fp16 hi")
    same_words(lo, want["lo"], what + " fp16 lo", want["lo"])
    same_words(ph, want["ph"], what + " bf16 hi (permuted)")
    same_words(pl, want["pl"], what + " bf16 lo (permuted)")


@pytest.mark.parametrize("name", R.SPLIT_SETS)
@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("rows_pad", R.SPLIT_ROWS)
def test_split_workspaces_bit_for_bit(rows_pad, kp, name):
    """The fp16 hi / lo words, the permuted bf16 hi / lo words and the scale header of both entry points equal the restatement bit for bit:
    rows_pad of 1, 4 and 129 blocks of 32 (4128 x 64 words pass the 4096 x 256 threads of the split's grid: its loop strides), the pair
    taken with a partner of another height, column maxima spanning 2^40, a dead column in each factor, an all-zero pair.  (On an MI355X
    every word agrees, the subnormal fp16 lo addends of the `span` set included: the conversion does not flush them.)"""
    from pybmf_amd import _lib as L
    b_pad = R.SPLIT_ROWS[(R.SPLIT_ROWS.index(rows_pad) + 1) % len(R.SPLIT_ROWS)]
    A, B = R.split_factor(rows_pad, kp, name, 0), R.split_factor(b_pad, kp, name, 1)
    Ad, Bd = dev(A), dev(B)
    wsA, wsB = new_ws(rows_pad, kp), new_ws(b_pad, kp)
    L.check(L.lib.bmf_link_split_pair(L.ptr(Ad), rows_pad, L.ptr(Bd), b_pad, kp, L.ptr(wsA), L.ptr(wsB), stream()), "bmf_link_split_pair")
    headA, headB, S, T = R.pair_headers(A, B)
    check_ws(wsA, A, kp, S, headA, f"pair A {rows_pad}x{kp} {name}")
    check_ws(wsB, B, kp, T, headB, f"pair B {b_pad}x{kp} {name}")
    ws1 = new_ws(rows_pad, kp)
    L.check(L.lib.bmf_link_split(L.ptr(Ad), rows_pad, kp, L.ptr(ws1), stream()), "bmf_link_split")
    head1, S1 = R.single_header(A)
    check_ws(ws1, A, kp, S1, head1, f"single {rows_pad}x{kp} {name}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. bmf_colsum_fill
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def colsum_input(rows, kp, integers):
    rs = np.random.RandomState(rows + kp + integers)
    F = rs.randint(0, 8, size=(rows, kp)).astype(np.float32) if integers else (rs.standard_normal((rows, kp)) * 3).astype(np.float32)
    want = R.colsum_ref(F)
    return F, dev(F), want, R.colsum_bound(F, want)


@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("out_rows", R.COLSUM_OUT_ROWS)
@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_colsum_fill_every_entry(rows, out_rows, kp):
    """Column sums against math.fsum -- exact on integer-valued data, else within half an fp32 ulp plus rows 2^-53 sum |v| -- and every one
    of the out_rows x kp entries of `out` equal to colsum: the fp64 partials that lived in the head of `out` are gone."""
    from pybmf_amd import _lib as L
    assert R.colsum_blocks(rows, out_rows) is not None
    for integers in (True, False):
        F, Fd, want, bound = colsum_input(rows, kp, integers)
        colsum = torch.full((kp,), SENTINEL, device="cuda")
        out = torch.full((out_rows + 1, kp), SENTINEL, device="cuda")
        L.check(L.lib.bmf_colsum_fill(L.ptr(Fd), rows, kp, L.ptr(colsum), L.ptr(out), out_rows, stream()), "bmf_colsum_fill")
        cs, o = colsum.cpu().numpy(), out.cpu().numpy()
        assert (o[out_rows] == SENTINEL).all()
        assert (o[:out_rows] == cs[None, :]).all()
        err = np.abs(cs.astype(np.float64) - want)
        if integers:
            assert (err == 0).all()
        else:
            note(("colsum", f"kp{kp}"), gate=(err / bound).max())
            assert (err <= bound).all(), (err / bound).max()


def test_colsum_fill_refuses_a_single_output_row():
    from pybmf_amd import _lib as L
    F, Fd, _, _ = colsum_input(65, 32, True)
    colsum, out = torch.full((32,), SENTINEL, device="cuda"), torch.full((2, 32), SENTINEL, device="cuda")
    assert L.lib.bmf_colsum_fill(L.ptr(Fd), 65, 32, L.ptr(colsum), L.ptr(out), 1, stream()) == -1
    assert "out is too small" in last_error()
    assert (colsum.cpu().numpy() == SENTINEL).all() and (out.cpu().numpy() == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "16"])
def test_pass_refuses_bad_arguments_and_launches_nothing(kind):
    o = oriented(130, 515, 40, "moderate", False)
    name = "bmf_link_pass" if kind == "f32" else "bmf_link_pass16"
    splits, stride = R.splits_for(130, 515), o["rows_pad"] * o["kp"]
    assert splits == 2
    shifted = off(o["Fsd"], 4) if kind == "f32" else off(o["ws_s"], 2)
    shifted_o = off(o["Fod"], 4) if kind == "f32" else off(o["ws_o"], 2)
    bad = [(dict(splits=1), "splits=1"), (dict(splits=3), "splits=3"), (dict(stride=stride - 1), "slab_stride too small"),
           (dict(self=shifted), "16-byte aligned"), (dict(other=shifted_o), "16-byte aligned"), (dict(link=0), "link must be"),
           (dict(link=3), "link must be"), (dict(den=None), "needs a den buffer")]
    for over, text in bad:
        rc, num, den = run_pass(o, kind, R.LINK_SIGMOID, 10.0, over)
        assert rc == -1, (over, rc)
        assert name + ":" in last_error() and text in last_error(), (over, last_error())
        assert (num == SENTINEL).all() and (den == SENTINEL).all()               # nothing was launched
    rc, num, den = run_pass(o, kind, R.LINK_KL, 1.0, dict(den=None))                  # KL needs no den
    assert rc == 0 and (num[:splits] >= 0).all()


def test_sums_and_split_refuse_bad_arguments():
    from pybmf_amd import _lib as L
    f = case_factors(33, 65, 5, "moderate")
    bits, _, ldx, _ = case_bits(33, 65)
    sums = dev(PRESET.copy())
    for fn, a, b, name in ((L.lib.bmf_link_sums, f["Ud"], f["Vd"], "bmf_link_sums:"), (L.lib.bmf_link_sums16, f["wsU"], f["wsV"], "bmf_link_sums16:")):
        for link in (0, 3):
            assert fn(L.ptr(bits), f["m_pad"], ldx, 33, 65, L.ptr(a), L.ptr(b), f["n_pad"], f["kp"], link, 1.0, None, L.ptr(sums), stream()) == -1
            assert name in last_error() and "link must be" in last_error()
        assert fn(L.ptr(bits), f["m_pad"], 2, 33, 65, L.ptr(a), L.ptr(b), f["n_pad"], f["kp"], R.LINK_KL, 1.0, None, L.ptr(sums), stream()) == -1
        assert name in last_error() and "bad shape" in last_error()              # ldx * 32 < n
    assert L.lib.bmf_link_sums16(L.ptr(bits), f["m_pad"], ldx, 33, 65, off(f["wsU"], 2), L.ptr(f["wsV"]), f["n_pad"], f["kp"], R.LINK_KL, 1.0, None,
                                 L.ptr(sums), stream()) == -1
    assert "16-byte aligned" in last_error()
    assert np.array_equal(sums.cpu().numpy(), PRESET)
    F = dev(R.split_factor(32, 32, "moderate", 0))
    ws = new_ws(33, 32)
    for args, text in (((L.ptr(F), 32, 32, off(ws, 2)), "16-byte aligned"), ((L.ptr(F), 33, 32, L.ptr(ws)), "multiple of 32"),
                       ((L.ptr(F), 32, 48, L.ptr(ws)), "kp 32 or 64")):
        assert L.lib.bmf_link_split(*args, stream()) == -1 and "bmf_link_split:" in last_error() and text in last_error()
    assert L.lib.bmf_link_split_pair(L.ptr(F), 32, L.ptr(F), 32, 32, L.ptr(ws), off(ws, 2), stream()) == -1
    assert "bmf_link_split_pair:" in last_error() and "16-byte aligned" in last_error()
    assert (ws.cpu().numpy().view(np.uint16) == 0x5A5A).all()
    assert L.lib.bmf_link_splits(0, 5) == -1 and "bmf_link_splits:" in last_error()
