"""bmf_nmf_cd_sweep (csrc/nmf_cd.hip) called directly, cell by cell against the literal sweep of tests/nmf_ref.py, both fed the same
fp64 Gram and the same fp32 numerator slabs.

Device and reference run the same fp64 operations; the only freedom the contract leaves is the order in which
at most 64 terms are added, carried through at most 64 sequential coordinates -- 64 * 64 * 2^-53 = 4.5e-13 of the largest entry; the
gate is 1e-11 of it (a 20-fold margin).  The zero pattern must match exactly, which is meaningful because the test asserts, on the
CPU, that no clamp decision of its inputs is closer than 1e-5 max|W| to 0.

Inputs per shape: W with cells that are exactly 0, some of them under a negative gradient (they become positive) and some under a
positive one (they stay 0); a Gram with a zero row, column and diagonal entry (the hess == 0 branch) where k >= 5; slabs and Gram
poisoned with NaN beyond `rows` and `k`, the padding of F64 on entry too (the ABI says none of it counts); output buffers pre-filled
with a marker.
"""
import numpy as np
import pytest

import nmf_ref

pytestmark = pytest.mark.gpu

ROWS = (1, 127, 128, 129, 3 * 128 + 5)
KS = (1, 5, 32, 33, 64)
MARK = -7.0


def make_inputs(rows, k, splits, seed):
    """(W, HHt, slabs [splits][rows_pad][kp] with NaN padding, rows_pad, kp)"""
    rng = np.random.RandomState(seed)
    kp = 32 if k <= 32 else 64
    rows_pad = -(-rows // 128) * 128
    W = rng.rand(rows, k) + 0.05
    W[rng.rand(rows, k) < 0.3] = 0.0
    H = rng.rand(max(2 * k, 8), k) * (rng.rand(max(2 * k, 8), k) < 0.6)
    HHt = H.T @ H
    target = rng.rand(rows, k) * (rng.rand(rows, k) < 0.6)     # the rows of W the numerators pull towards
    XHt = target @ HHt + 0.05 * rng.rand(rows, k)
    if k >= 5:
        z = k // 2
        HHt[z, :] = 0.0
        HHt[:, z] = 0.0
    # the numerators as `splits` fp32 slabs whose fp64 sum in slab order is what both sides use
    parts = rng.dirichlet(np.ones(splits), size=(rows, k)).transpose(2, 0, 1) * XHt[None]
    slabs = np.full((splits, rows_pad, kp), np.nan, dtype=np.float32)
    slabs[:, :rows, :k] = parts.astype(np.float32)
    return W, HHt, slabs, rows_pad, kp


def reference(W, HHt, slabs):
    rows, k = W.shape
    XHt = nmf_ref.sum_slabs(slabs[:, :rows, :k])
    margins, Wn = [], W.copy()
    viol = nmf_ref.cd_sweep(Wn, HHt, XHt, margins)
    return Wn, viol, (min(margins) if margins else np.inf)


def inputs_with_margin(rows, k, splits):
    """The first seed whose clamp decisions all keep 1e-5 max|W| away from 0 (decided on the CPU, from the reference alone)."""
    for seed in range(100):
        W, HHt, slabs, rows_pad, kp = make_inputs(rows, k, splits, 1000 * rows + 10 * k + splits + 7919 * seed)
        Wn, viol, margin = reference(W, HHt, slabs)
        if margin >= 1e-5:
            return W, HHt, slabs, rows_pad, kp, Wn, viol, margin
    raise AssertionError("no seed with a clamp margin of 1e-5")


def run_device(W, HHt, slabs, rows_pad, kp):
    import torch
    from pybmf_amd import _lib as L
    rows, k = W.shape
    splits = slabs.shape[0]
    dev = "cuda:0"
    F64h = np.full((rows_pad, kp), np.nan)      # (the padding of F64 is ignored on entry as well)
    F64h[:rows, :k] = W
    Gh = np.full((kp, kp), np.nan)
    Gh[:k, :k] = HHt
    F64 = torch.from_numpy(F64h).to(dev)
    F = torch.full((rows_pad, kp), MARK, dtype=torch.float32, device=dev)
    G = torch.from_numpy(Gh).to(dev)
    num = torch.from_numpy(slabs).to(dev)
    nb = rows_pad // 128
    guard = 5
    blockmax = torch.full((nb * kp + guard,), MARK, dtype=torch.float32, device=dev)
    viol = torch.full((nb + guard,), MARK, dtype=torch.float64, device=dev)
    rc = L.lib.bmf_nmf_cd_sweep(L.ptr(F64), L.ptr(F), rows_pad, rows, k, kp, L.ptr(num), rows_pad * kp, splits, L.ptr(G), L.ptr(blockmax),
                                L.ptr(viol), None)
    L.check(rc, "bmf_nmf_cd_sweep")
    torch.cuda.synchronize()
    assert np.array_equal(num.cpu().numpy(), slabs, equal_nan=True) and np.array_equal(G.cpu().numpy(), Gh, equal_nan=True)
    bm, vl = blockmax.cpu().numpy(), viol.cpu().numpy()
    assert (bm[nb * kp:] == MARK).all() and (vl[nb:] == MARK).all()
    return F64.cpu().numpy(), F.cpu().numpy(), bm[: nb * kp].reshape(nb, kp), vl[:nb]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("rows", ROWS)
def test_sweep_matches_the_literal_reference_cell_by_cell(rows, k):
    for splits in (1, 3):
        W, HHt, slabs, rows_pad, kp, want, want_viol, margin = inputs_with_margin(rows, k, splits)
        assert margin >= 1e-5
        if rows >= 127 and k >= 5:   # both kinds of exact zeros are in the input, outside the column that hess == 0 leaves alone
            was_zero = W == 0
            was_zero[:, k // 2] = False
            assert (was_zero & (want > 0)).any() and (was_zero & (want == 0)).any()
        if k >= 5:
            assert HHt[k // 2, k // 2] == 0 and np.array_equal(want[:, k // 2], W[:, k // 2])   # hess == 0: the column is left alone
        F64, F, blockmax, viol = run_device(W, HHt, slabs, rows_pad, kp)
        got = F64[:rows, :k]
        scale = max(np.abs(want).max(), 1e-300)
        print(f"rows={rows} k={k} splits={splits}: max |dW| / max|W| = {np.abs(got - want).max() / scale:.3g}, "
              f"violation rel = {abs(viol.sum() - want_viol) / max(want_viol, 1e-300):.3g}, clamp margin = {margin:.3g}")
        assert np.isfinite(F64).all() and np.isfinite(F).all()
        assert np.array_equal(got == 0, want == 0)
        assert np.abs(got - want).max() <= 1e-11 * scale
        assert abs(viol.sum() - want_viol) <= 1e-11 * want_viol
        # padding rows and columns: exact zeros in both copies
        assert not F64[rows:].any() and not F64[:, k:].any() and not F[rows:].any() and not F[:, k:].any()
        # the shadow and the block maxima follow from the device's own fp64 result exactly
        assert np.array_equal(F, F64.astype(np.float32))
        assert np.array_equal(blockmax, nmf_ref.block_maxima(got, rows_pad, kp))


def test_violation_partials_are_per_block_and_padding_adds_nothing():
    rows, k = 3 * 128 + 5, 33
    W, HHt, slabs, rows_pad, kp, want, want_viol, _ = inputs_with_margin(rows, k, 3)
    _, _, _, viol = run_device(W, HHt, slabs, rows_pad, kp)
    XHt = nmf_ref.sum_slabs(slabs[:, :rows, :k])
    for b in range(rows_pad // 128):
        lo, hi = 128 * b, min(128 * b + 128, rows)
        part = nmf_ref.cd_sweep(W[lo:hi].copy(), HHt, XHt[lo:hi])
        assert abs(viol[b] - part) <= 1e-11 * part


def test_all_zero_factor_and_gram_take_the_hess_zero_branch():
    """What the all-zero matrix gives under init 'random': nothing moves, the violation is exactly 0."""
    rows, k, kp, rows_pad = 130, 3, 32, 256
    slabs = np.zeros((2, rows_pad, kp), dtype=np.float32)
    F64, F, blockmax, viol = run_device(np.zeros((rows, k)), np.zeros((k, k)), slabs, rows_pad, kp)
    assert not F64.any() and not F.any() and not blockmax.any() and not viol.any()
