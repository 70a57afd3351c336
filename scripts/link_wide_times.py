"""Timing of the link models at a rank above 64 on one MI355X: iterations per second of PNLPF and of WNMF with the Kullback-Leibler loss
at a planted 20 000 x 5 000, k = 128 on the two-block engine (pybmf_amd/link_wide.py, exact-fp32 MFMA) beside k = 64 on
engine.LinkMUEngine with mfma='f32' and mfma='bf16'.  The same stepwise calls for all three (engine.update, no scalars read), warm-up
first, the device synchronised around the timed window.

    python scripts/link_wide_times.py [out.txt] [m n]        (the timing lines of profiles/link_wide_times.txt are its output)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from pybmf_amd import _lib as L
from pybmf_amd.engine import BitMatrix
from pybmf_amd.generators import PlantedBooleanOnDevice
from pybmf_amd.link_wide import link_engine

out = open(sys.argv[1] if len(sys.argv) > 1 else "link_wide_times.txt", "w")
m, n = (int(v) for v in sys.argv[2:4]) if len(sys.argv) > 3 else (20000, 5000)
CMD = "python " + " ".join([os.path.relpath(os.path.abspath(sys.argv[0]), ROOT)] + sys.argv[1:])   # the command as it was run


def say(*parts):
    line = " ".join(str(x) for x in parts) + "   [" + CMD + "]"
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


X = BitMatrix(PlantedBooleanOnDevice(m, n, 64, density=(0.067, 0.067), seed=1000, noise=(0.05, 0.01), noise_seed=2000), "cuda:0")
say(f"matrix {m} x {n}, ones {X.sum_local}")
rates = {}
for model, link, mode in (("PNLPF", L.LINK_SIGMOID, L.MODE_PENALTY), ("WNMF-KL", L.LINK_KL, L.MODE_WNMF)):
    for k, mfma in ((128, None), (64, "f32"), (64, "bf16")):
        rs = np.random.RandomState(k)
        s = np.sqrt(0.5 / k) / 0.8
        U0, V0 = np.abs(rs.standard_normal((m, k))) * s + 1e-3, np.abs(rs.standard_normal((n, k))) * s + 1e-3
        eng = link_engine(X, k, link, mode, lamda=10.0, mfma=mfma)
        eng.load_factors(U0, V0)
        eng.prepare()
        for _ in range(3):
            eng.update(1.0)
        torch.cuda.synchronize()
        reps = 10
        t0 = time.perf_counter()
        for _ in range(reps):
            eng.update(1.0)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        rates[(model, k, mfma)] = 1.0 / dt
        say(f"{model} k = {k} on {type(eng).__name__}" + (f"(mfma='{mfma}')" if mfma else " (exact-fp32 MFMA)") +
            f": {dt * 1e3:.2f} ms per iteration (V and U updates), {1.0 / dt:.1f} iterations/s")
        del eng
    say(f"{model}: k = 128 runs at {rates[(model, 128, None)] / rates[(model, 64, 'f32')]:.2f} x the rate of k = 64 on the same fp32 MFMA, "
        f"{rates[(model, 128, None)] / rates[(model, 64, 'bf16')]:.2f} x the rate of k = 64 on the 16-bit MFMAs")
out.close()
