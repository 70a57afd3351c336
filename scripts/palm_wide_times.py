"""ELBMF at a rank above 64 beside k = 64, on one MI355X: iterations/s at 20 000 x 5 000 (planted Boolean, beta = 0) of the two-block
engine at k = 128 (palm_wide.WidePalmEngine, stepwise: one synchronising read per iteration), of the k = 64 engine driven the same
way, and of the k = 64 loop as ELBMF.fit runs it (one C call per iteration, scalars read one iteration late) -- device events around
40 iterations after 5 of warm-up, three legs per configuration, alternating; and bmf_sym_norms_wide (128 x 128) beside bmf_sym_norms
(64 x 64) on the Grams of those runs, 200 back-to-back calls.  The clock state is read (never set) before the run.  No gate: nobody
had timed these models above k = 64.

    python scripts/palm_wide_times.py [out.txt]        (profiles/palm_wide_times.txt is its output)
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from pybmf_amd import _lib as L
from pybmf_amd.engine import BitMatrix
from pybmf_amd.palm import PalmEngine
from pybmf_amd.palm_wide import WidePalmEngine

out = open(sys.argv[1] if len(sys.argv) > 1 else "palm_wide_times.txt", "w")
def say(*a):
    s = " ".join(str(x) for x in a); print(s, flush=True); out.write(s + "\n"); out.flush()

say("command: python scripts/palm_wide_times.py   (torch", torch.__version__, ",", torch.cuda.get_device_name(0), ")")
try:
    r = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=60)
    keep = [l for l in r.stdout.splitlines() if ("GPU[0]" in l and ("sclk" in l or "mclk" in l or "fclk" in l or "Performance" in l))]
    say("clock state before (rocm-smi, GPU 0, read only):"); [say("   ", l.strip()) for l in keep] if keep else say("    (no clock lines reported)")
except Exception as e:  # noqa: BLE001
    say("clock state: rocm-smi not available:", type(e).__name__)

m, n = 20000, 5000
rs = np.random.RandomState(0)
X = ((rs.rand(m, 16) < 0.2).astype(np.int32) @ (rs.rand(16, n) < 0.2).astype(np.int32) > 0).astype(np.uint8)
B = BitMatrix(X, "cuda:0")
sched = lambda t: (0.01, 0.02 * 1.02 ** t)

def stepwise(eng, t0, T):
    for t in range(t0, t0 + T):
        l1, l2 = sched(t)
        eng.step("U", l1, l2, l1, l2); eng.step("V", l1, l2, l1, l2); eng.refresh("U"); eng.refresh("V"); eng.scalars()

def pipelined(eng, t0, T):   # as ELBMF.iPALM drives it: iteration t + 1 enqueued before row t is read
    eng.iterate(t0, *sched(t0), *sched(t0))
    for t in range(t0, t0 + T):
        eng.iterate(t + 1, *sched(t + 1), *sched(t + 1)); eng.row(t)

engs = {}
for name, k, cls in (("k=128 two-block stepwise", 128, WidePalmEngine), ("k=64 stepwise", 64, PalmEngine), ("k=64 one C call per iteration", 64, PalmEngine)):
    e = cls(B, k, L.PALM_ELBMF, beta=0.0)
    e.load_factors(rs.rand(m, k) * 0.3, rs.rand(n, k) * 0.3)
    engs[name] = (e, pipelined if "C call" in name else stepwise)
T, W = 40, 5
rates = {nm: [] for nm in engs}
pos = {nm: 0 for nm in engs}
for leg in range(3):
    for nm, (e, fn) in engs.items():
        fn(e, pos[nm], W); pos[nm] += W + 1
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(e, pos[nm], T); e1.record(); torch.cuda.synchronize()
        pos[nm] += T + 1
        rates[nm].append(T / (e0.elapsed_time(e1) * 1e-3))
say(f"ELBMF, {m} x {n} Boolean, beta = 0, int8 x3 operands; {T} iterations per leg after {W} warm-up, three legs alternating (iterations/s):")
for nm, r in rates.items():
    say("    %-32s %s   median %.1f" % (nm, " ".join("%.1f" % x for x in r), sorted(r)[1]))

def time_calls(fn, reps=200):
    for _ in range(20): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps
w, nrw = engs["k=128 two-block stepwise"][0], engs["k=64 stepwise"][0]
o = torch.zeros(2, dtype=torch.float64, device="cuda")
for leg in range(3):
    a = time_calls(lambda: L.lib.bmf_sym_norms_wide(L.ptr(w.GV64), L.ptr(o), None))
    b = time_calls(lambda: L.lib.bmf_sym_norms(L.ptr(nrw.GV64), 64, L.ptr(o), None))
    say("    bmf_sym_norms_wide (128 x 128 Gram of V, k = 128): %.1f us per call    bmf_sym_norms (64 x 64, k = 64): %.1f us per call   (200 back-to-back calls, incl. launch)" % (a, b))
G = torch.from_numpy(np.linalg.qr(rs.standard_normal((128, 128)))[0]).cuda()
Gs = (G * torch.linspace(1, 0.5, 128, dtype=torch.float64, device="cuda")) @ G.T
say("    bmf_sym_norms_wide on a matrix with no dominant direction (eigenvalues 1 .. 0.5, all 32 squarings): %.1f us per call" %
    time_calls(lambda: L.lib.bmf_sym_norms_wide(L.ptr(Gs.contiguous()), L.ptr(o), None)))
out.close()
