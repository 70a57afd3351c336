"""What the rank 64 < k <= 128 engines share (pybmf_amd/blocks.py), the parts that need no GPU: a host factor into two zero-padded
64-column blocks and back, the argument block of bmf_mu_epilogue as the three MU engines fill it, and every refusal of a rank above
64 with its text."""
import itertools

import numpy as np
import pytest
import torch

from pybmf_amd import _lib as L
from pybmf_amd import blocks as B

PAD = 512


# ---- split and join ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [65, 72, 128])
@pytest.mark.parametrize("rows", [1, 37, 512])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_split_and_join_round_trip_with_zero_padding(k, rows, dtype):
    F = np.random.RandomState(1000 * k + rows).rand(rows, k) + 0.5     # (no zero among the real entries)
    blocks = [torch.full((PAD, B.BK), 7.0, dtype=dtype) for _ in range(2)]      # stale content: the split has to clear it
    B.split_into(blocks, F)
    want = F.astype(np.float64 if dtype == torch.float64 else np.float32)
    back = B.join(blocks, rows, k)
    assert back.shape == (rows, k) and back.dtype == want.dtype and (back == want).all()
    b0, b1 = (t.numpy() for t in blocks)
    assert (b0[:rows] == want[:, :64]).all() and (b1[:rows, : k - 64] == want[:, 64:]).all()      # block 1: the k - 64 real columns
    assert (b0[rows:] == 0).all() and (b1[rows:] == 0).all() and (b1[:, k - 64:] == 0).all()
    assert np.count_nonzero(b1) == rows * (k - 64) and np.count_nonzero(b0) == rows * 64


# ---- the EpilogueArgs filler ------------------------------------------------------------------------------------------------------
M, N, K, SPLITS = 37, 20, 72, 3
M_PAD, N_PAD = 512, 256


class Blocks(B.BlockEngine):
    thr = (0.25, 0.75)


@pytest.fixture(scope="module")
def eng():
    e = Blocks()
    e._alloc_blocks(M, N, M_PAD, N_PAD, "cpu", K)
    e.partU, e.partV = e._blocks((M_PAD // 128, 2), torch.float64), e._blocks((N_PAD // 128, 2), torch.float64)
    e._extend_sides(U=dict(part=e.partU), V=dict(part=e.partV))
    return e


def fields(a):
    return {name: (getattr(a, name) or 0) for name, _ in L.EpilogueArgs._fields_}      # (a null pointer field reads as None)


@pytest.mark.parametrize("case", ["mu", "masked", "masked-prepare", "link"])
@pytest.mark.parametrize("which", ["U", "V"])
@pytest.mark.parametrize("b", [0, 1])
def test_epilogue_args_field_by_field(eng, case, which, b):
    rows, rows_pad = (M, M_PAD) if which == "U" else (N, N_PAD)
    F64, F, rb, cb, part, thr = ((eng.U64, eng.U, eng.ubits, eng.ucolbits, eng.partU, 0.25) if which == "U" else
                                 (eng.V64, eng.V, eng.vbits, eng.vcolbits, eng.partV, 0.75))
    den = [torch.zeros((rows_pad, 64), dtype=torch.float32) for _ in range(2)]
    splits = {"mu": SPLITS, "masked": 1, "masked-prepare": 1, "link": 5}[case]
    num = [torch.zeros((splits, rows_pad, 64), dtype=torch.float32) for _ in range(2)]
    mode = L.MODE_PREPARE if case == "masked-prepare" else (L.MODE_WNMF if case == "link" else L.MODE_PENALTY)
    reg = 0.0 if case == "masked-prepare" else 1.5
    a = eng._epilogue_args(which, b, mode, reg, None if case == "masked-prepare" else num, splits, den)
    assert fields(a) == dict(
        F64=F64[b].data_ptr(), F=F[b].data_ptr(), rows_pad=rows_pad, rows=rows, k=[64, 8][b], kp=64,
        num=0 if case == "masked-prepare" else num[b].data_ptr(), slab_stride=rows_pad * 64, splits=splits,
        G=0, reg=reg, mode=mode, thr=thr, terms=0,
        panel=0, ldp=rows_pad, rowbits=rb[b].data_ptr(), colbits=cb[b].data_ptr(), ldcb=rows_pad // 32,
        partials=part[b].data_ptr(), stop=0, den=den[b].data_ptr(), blockmax=0, num_block_stride=0,
        planes=0, plane_scale=0, limbs=0, _pad0=0)
    assert eng.kb == [64, 8] and (eng.nb, eng.kp) == (2, 64)


def test_count_tuple(eng):
    eng.sum_x = 100.0
    assert eng._count_tuple(60, 7) == (60, 7, 40, M * N - 107)


# ---- check_wide: every refusal, with its text ------------------------------------------------------------------------------------------
ABOVE = "this build supports k <= 128"
TEXTS = {   # what: (sharded, data that is not 0 / 1, mfma='bf16'); None: accepted
    "mu": ("a rank above 64 runs on one GPU, on Boolean (0/1) data", "a rank above 64 runs on one GPU, on Boolean (0/1) data", None),
    "link": ("a rank above 64 runs on one GPU (row sharding needs k <= 64)",
             "the link models at a rank above 64 take Boolean (0/1) data; real-valued data needs k <= 64",
             "the link passes at a rank above 64 run on the exact-fp32 MFMA only (mfma='bf16' needs k <= 64)"),
    "palm": ("a rank above 64 runs on one GPU", None, None),
    "threshold": ("a rank above 64 runs on one GPU (a sharded run needs k <= 64)",
                  "BinaryMFThreshold at a rank above 64 takes Boolean (0/1) data; real-valued data needs k <= 64", None),
}


def expected(what, k, sharded, boolean, mfma):
    """The text a picker or model of family `what` refuses (k, sharded, boolean, mfma) with, or None."""
    if k > 128:
        return ABOVE
    if k <= 64:
        return None
    for refused, text in zip((sharded, not boolean, mfma == "bf16"), TEXTS[what]):
        if refused and text:
            return text
    return None


@pytest.mark.parametrize("what", sorted(TEXTS))
def test_check_wide_table(what):
    for k, sharded, boolean, mfma in itertools.product((1, 64, 65, 72, 128, 129, 200), (False, True), (True, False), (None, "fp32", "bf16")):
        text = expected(what, k, sharded, boolean, mfma)
        if text is None:
            assert B.check_wide(k, sharded=sharded, boolean=boolean, mfma=mfma, what=what) is None
        else:
            with pytest.raises(NotImplementedError) as e:
                B.check_wide(k, sharded=sharded, boolean=boolean, mfma=mfma, what=what)
            assert str(e.value) == f"k={k}: {text}", (k, sharded, boolean, mfma)


def test_check_wide_accepts_64_and_65_to_128():
    for what in TEXTS:
        for k in [64] + list(range(65, 129)):
            assert B.check_wide(k, what=what) is None
    for what in ("mu engine", "link engine", "palm engine"):
        for k in range(65, 129):
            assert B.check_wide(k, what=what) is None


def test_constructors_and_pickers_refuse_before_the_data_is_touched():
    """Every caller of check_wide with None in the place of its data, with the text it has always had."""
    from pybmf_amd.link_wide import WideLinkMUEngine, check_wide_link, link_engine
    from pybmf_amd.palm_wide import WidePalmEngine, palm_engine
    from pybmf_amd.wide import WideMaskedMUEngine, WideMUEngine
    two = "the two-block engine takes 64 < k <= 128"
    cases = [
        (lambda k: WideMUEngine(None, k), {64: two, 129: two}),
        (lambda k: WideMaskedMUEngine(None, k, L.MODE_PENALTY), {64: two, 129: two}),
        (lambda k: WideLinkMUEngine(None, k, L.LINK_SIGMOID, L.MODE_PENALTY), {64: "the two-block link engine takes 64 < k <= 128",
                                                                                129: "the two-block link engine takes 64 < k <= 128"}),
        (lambda k: WidePalmEngine(None, k, L.PALM_ELBMF), {64: two, 129: ABOVE}),
        (lambda k: palm_engine(None, k, L.PALM_ELBMF), {129: ABOVE}),
        (lambda k: palm_engine(None, k, L.PALM_ELBMF, sharded=True), {72: TEXTS["palm"][0], 129: ABOVE}),
        (lambda k: link_engine(None, k, L.LINK_KL, L.MODE_WNMF), {129: ABOVE}),
        (lambda k: link_engine(None, k, L.LINK_KL, L.MODE_WNMF, sharded=True), {72: TEXTS["link"][0]}),
        (lambda k: link_engine(None, k, L.LINK_KL, L.MODE_WNMF, boolean=False), {72: TEXTS["link"][1]}),
        (lambda k: link_engine(None, k, L.LINK_KL, L.MODE_WNMF, mfma="bf16"), {72: TEXTS["link"][2]}),
        (lambda k: check_wide_link(k, sharded=True, boolean=False, mfma="bf16"), {72: TEXTS["link"][0], 129: ABOVE}),
    ]
    for call, by_k in cases:
        for k, text in by_k.items():
            with pytest.raises(NotImplementedError) as e:
                call(k)
            assert str(e.value) == f"k={k}: {text}"
    assert check_wide_link(64, sharded=True, boolean=False, mfma="bf16") is None
