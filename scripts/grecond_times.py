"""Timing of the GreConD engine at 6040 x 3706 on one MI355X: per-launch time of bmf_concept_scan (device events) for a first and a
late sweep with the words it reads, launches and accepted candidates per concept, wall time of a k = 20 fit and of fixture case b.

    python scripts/grecond_times.py [out.txt]        (profiles/grecond_times.txt is its output)
"""
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
from scipy.sparse import csr_matrix

from pybmf_amd.bitset import unpack_bits
from pybmf_amd.engine import BitMatrix
from pybmf_amd.grecond import ConceptEngine
from pybmf_amd.models import GreConD

QUIET = dict(task="reconstruction", show_logs=False, show_result=False, save_model=False)
out = open(sys.argv[1] if len(sys.argv) > 1 else "grecond_times.txt", "w")


def say(*parts):
    line = " ".join(str(x) for x in parts)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def planted_ml1m():
    """The matrix of tests/test_grecond_gpu.py::planted_ml1m: 26 planted rectangles, 0.1 % of the cells flipped, about 4.7 % ones."""
    rng = np.random.RandomState(2310)
    m, n, k = 6040, 3706, 26
    U, V = rng.rand(m, k) < 0.06, rng.rand(n, k) < 0.03
    X = (U.astype(np.float32) @ V.astype(np.float32).T) > 0
    X ^= rng.rand(m, n) < 0.001
    return X.astype(np.uint8)


def words_read(X, W, best_u, cands):
    """Global words one scan reads by the kernel's own rule: a (group of 16 candidates, column) pair reads 64-word chunks of Xt[c]
    until no candidate of the group is alive (candidates with an empty u_j are never alive), and all chunks of Xrs_t[c] when one is
    left.  Returns (Xt words, Xrs_t words, pairs (j, c) with a non-empty u_j inside column c)."""
    m, n = X.shape
    dev = "cuda:0"
    Xb = torch.from_numpy(X.astype(np.float32)).to(dev)
    ub = torch.from_numpy(unpack_bits(best_u, m).astype(np.float32)).to(dev)
    cidx = torch.from_numpy(np.asarray(cands, dtype=np.int64)).to(dev)
    groups = (len(cands) + 15) // 16
    pad = torch.zeros((groups * 16 - len(cands), n), dtype=torch.bool, device=dev)
    alive = ((Xb[:, cidx] * ub[:, None]).sum(0) > 0)[:, None].expand(len(cands), n).clone()
    chunks = (W + 63) // 64
    x_words = 0
    for ch in range(chunks):
        x_words += int(torch.cat([alive, pad]).view(groups, 16, n).any(1).sum().item()) * 64
        r0, r1 = ch * 2048, min((ch + 1) * 2048, m)
        if r0 < m:
            U = Xb[r0:r1, cidx].T * ub[r0:r1]
            alive &= (U @ (1 - Xb[r0:r1])) == 0
    rs_words = int(torch.cat([alive, pad]).view(groups, 16, n).any(1).sum().item()) * 64 * chunks
    return x_words, rs_words, int(alive.sum().item())


def time_scan(eng, X, label, best_u, cands, reps=20):
    eng.set_search_state(best_u, cands)
    for _ in range(3):
        eng.launch_scan(0, len(cands), 1 << 60)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.launch_scan(0, len(cands), 1 << 60)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    _, nu, _, _ = eng.scan_results(len(cands))
    x_words, rs_words, pairs = words_read(X, eng.W, best_u, cands)
    model = len(cands) * eng.n * eng.W * 2
    say(f"{label}: {len(cands)} candidates ({int((nu == 0).sum())} with an empty u_j), |best_u| = {int(unpack_bits(best_u, eng.m).sum())}: median "
        f"{ts[len(ts) // 2]:.0f} us (min {ts[0]:.0f}, max {ts[-1]:.0f}) per bmf_concept_scan (scan + pick kernels, device events, {reps} calls)")
    say(f"    words without early exit, candidates x n x W x 2 = {model:.3e}; global words read {x_words + rs_words:.3e} (Xt {x_words:.3e}, "
        f"Xrs_t {rs_words:.3e}); LDS word reads <= 16 x the Xt words; (j, c) pairs that pass the subset test: {pairs}")


def main():
    X = planted_ml1m()
    m, n = X.shape
    say(f"matrix: {m} x {n}, density {X.mean():.4f} (26 planted rectangles, 0.1 % flips, RandomState(2310)); one MI355X")
    eng = ConceptEngine(BitMatrix(X, "cuda:0"))
    say(f"W = m_pad / 32 = {eng.W} words per column bit row; 16 candidates per workgroup, 4 waves, 64-word chunks")
    all_rows = np.packbits(np.arange(eng.W * 32) < m, bitorder="little").view(np.uint32).copy()
    cols = eng.residual_columns()
    time_scan(eng, X, "first sweep (best_u = all rows)", all_rows, cols)
    s, u, v = eng.concept()
    say(f"concept 0: score {s}, shape [{int(unpack_bits(u, m).sum())}, {int(unpack_bits(v, n).sum())}], {eng.launches} launches, "
        f"{eng.accepted} accepted")
    rest = cols[~unpack_bits(v, eng.nvw * 32)[cols]]
    time_scan(eng, X, "late sweep (best_u = concept 0's rows)", u, rest)
    time_scan(eng, X, "late sweep, a block of 64", u, rest[:64])
    dense = np.packbits(np.arange(eng.W * 32) < m // 4, bitorder="little").view(np.uint32).copy()
    time_scan(eng, X, "middle sweep (best_u = the first quarter of the rows)", dense, cols)

    for block in (None, 512):
        e2 = ConceptEngine(BitMatrix(X, "cuda:0"))
        torch.cuda.synchronize()
        t0 = time.time()
        stats = []
        for _ in range(20):
            s, u, v = e2.concept(block=block)
            e2.apply(u, v)
            stats.append((e2.launches, e2.accepted))
        wall = time.time() - t0
        say(f"engine alone, 20 concepts, block = {block}: {wall:.3f} s; launches per concept {[a for a, _ in stats]}; "
            f"accepted per concept {[b for _, b in stats]}")

    with contextlib.redirect_stdout(io.StringIO()):
        t0 = time.time()
        GreConD(k=20).fit(X, **QUIET)
        wall = time.time() - t0
    say(f"GreConD(k=20).fit wall time: {wall:.2f} s (packing X, 20 concepts, lil factor updates, one log row per factor)")

    golden = os.path.join(ROOT, "tests", "golden")
    Xb = np.load(os.path.join(golden, "g23_grecond.npz"))["b_X"]
    meta = json.load(open(os.path.join(golden, "g23_grecond.json")))["cases"]["b"]
    for rep in range(2):
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.time()
            model = GreConD(k=meta["k"], tol=meta["tol"])
            model.fit(csr_matrix(Xb.astype(np.float64)), **QUIET)
            wall = time.time() - t0
        rows = len(model.logs["updates"])
        say(f"fixture case b (200 x 150, k=None, tol=0.02), run {rep}: {rows} concepts in {wall:.2f} s = {wall / rows * 1e3:.1f} ms per concept "
            f"(fit() wall time / rows); the reference took 0.25-0.38 s per concept on this case on a CPU host -- a different host")
    out.close()


if __name__ == "__main__":
    main()
