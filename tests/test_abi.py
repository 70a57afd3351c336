"""The C-ABI library: every symbol declared in include/bmf_hip.h is exported and bound, the ctypes mirrors of the two
structs have the C layout, and bad arguments are refused with an error code and a message (no compute, no GPU)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bmf_hip.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(bmf_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound():
    from pybmf_amd import _lib as L
    names = declared_functions()
    assert len(names) >= 20
    raw = C.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), f"{n} is declared in bmf_hip.h but missing from libbmf_hip.so"
        assert n in L.SIGNATURES, f"{n} has no ctypes signature in pybmf_amd/_lib.py"
    assert sorted(L.SIGNATURES) == names


def test_struct_layout_matches_c(tmp_path):
    from pybmf_amd import _lib as L
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n",'
                   'sizeof(bmf_epilogue_args), offsetof(bmf_epilogue_args, stop), sizeof(bmf_penalty_state),'
                   'offsetof(bmf_penalty_state, sum_x), offsetof(bmf_penalty_state, thr_u), offsetof(bmf_penalty_state, log),'
                   'sizeof(bmf_palm_args), offsetof(bmf_palm_args, beta), offsetof(bmf_palm_args, partials),'
                   'sizeof(bmf_palm_state), offsetof(bmf_palm_state, Xtiled), offsetof(bmf_palm_state, beta));return 0;}\n'
                   % HEADER)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(L.EpilogueArgs), L.EpilogueArgs.stop.offset, C.sizeof(L.PenaltyState), L.PenaltyState.sum_x.offset,
            L.PenaltyState.thr_u.offset, L.PenaltyState.log.offset, C.sizeof(L.PalmArgs), L.PalmArgs.beta.offset, L.PalmArgs.partials.offset,
            C.sizeof(L.PalmState), L.PalmState.Xtiled.offset, L.PalmState.beta.offset]
    assert got == want


def test_bad_arguments_are_refused_without_a_gpu():
    from pybmf_amd import _lib as L
    lib = L.lib
    assert lib.bmf_version() == 501 and lib.bmf_struct_bytes(0) > 0 and lib.bmf_struct_bytes(99) == -1
    assert lib.bmf_xf_bits(None, 512, 4, 4, None, 128, 3, 64, None, 512 * 64, 1, None) == -1
    assert b"null pointer" in lib.bmf_last_error()
    assert lib.bmf_xf_bits_slots(500, 4, 3, 64) == -1            # rows_pad not a multiple of 512
    assert lib.bmf_xf_bits_slots(512, 4, 3, 48) == -1            # kp must be 32 or 64
    assert lib.bmf_xf_bits_slots(100352, 640, 3, 64) >= 1
    assert lib.bmf_gram_partial(None, 512, 64, 64, None, 4, None) == -1
    assert lib.bmf_mu_epilogue(None, None) == -1
    st = L.PenaltyState()
    assert lib.bmf_penalty_prepare(C.byref(st), None) == -1 and b"struct_bytes" in lib.bmf_last_error()
    with pytest.raises(L.BmfError, match="struct_bytes"):
        L.check(lib.bmf_penalty_update(C.byref(st), 1.0, None), "bmf_penalty_update")
    assert sorted(lib.bmf_panel_pos(i) for i in range(128)) == list(range(128))
    assert lib.bmf_panel_pos(128) == -1


def test_host_only_launch_plan_queries():
    """bmf_residual_plan and bmf_residual_tiled_plan are host arithmetic: bad arguments are refused, and the grids are the ones worked
    out by hand from the rules in their launchers (csrc/residual.hip, csrc/resid_f32.hip).  bmf_xf_bits_i8_plan with an explicit
    compute-unit count is host arithmetic as well: its argument checks are here, its plans in tests/test_i8_plan_cpu.py."""
    from pybmf_amd import _lib as L
    lib = L.lib
    a, b = C.c_int(-7), C.c_int(-7)

    def plan(fn, x, y):
        a.value = b.value = -7
        assert fn(x, y, C.byref(a), C.byref(b)) == 0, lib.bmf_last_error()
        return a.value, b.value

    for fn, name, good in ((lib.bmf_residual_plan, b"bmf_residual_plan", (130, 70)), (lib.bmf_residual_tiled_plan, b"bmf_residual_tiled_plan", (64, 64))):
        assert fn(good[0], good[1], None, C.byref(b)) == -1 and name + b": null pointer" in lib.bmf_last_error()
        assert fn(good[0], good[1], C.byref(a), None) == -1 and name in lib.bmf_last_error()
        for bad in ((0, good[1]), (good[0], 0), (-64, good[1]), (good[0], -64), (1 << 31, good[1]), (good[0], 1 << 31)):
            a.value = b.value = -7
            assert fn(bad[0], bad[1], C.byref(a), C.byref(b)) == -1 and name in lib.bmf_last_error(), bad
            assert (a.value, b.value) == (-7, -7)                      # a refused call writes nothing
    for bad in ((100, 64), (64, 100), (63, 64), (64, 32)):
        assert lib.bmf_residual_tiled_plan(bad[0], bad[1], C.byref(a), C.byref(b)) == -1
    # residual: ceil(m / 128) row blocks; groups = min(ceil(1024 / row blocks), tiles); per = ceil(tiles / groups); groups = ceil(tiles / per)
    assert plan(lib.bmf_residual_plan, 1, 1) == (1, 1)
    assert plan(lib.bmf_residual_plan, 130, 70) == (3, 1)             # 2 row blocks -> up to 512 groups; 3 tiles, one each
    assert plan(lib.bmf_residual_plan, 1000, 333) == (11, 1)          # the largest shape of test_residual_sums: still one tile per group
    assert plan(lib.bmf_residual_plan, 128, 32768) == (1024, 1)       # 1 row block, 1024 tiles: the last shape with one tile per group
    assert plan(lib.bmf_residual_plan, 128, 32769) == (513, 2)        # 1025 tiles: 2 per group, 512 full groups and one of 1
    assert plan(lib.bmf_residual_plan, 129, 32769) == (342, 3)        # 2 row blocks -> 512 groups: 3 per group, 341 full groups and one of 2
    assert plan(lib.bmf_residual_plan, 8192, 33 * 32 - 5) == (11, 3)  # 64 row blocks -> 16 groups; 33 tiles: 3 per group, 11 full groups
    assert plan(lib.bmf_residual_plan, 8192, 34 * 32 - 5) == (12, 3)  # 34 tiles: 11 full groups and one of 1
    assert plan(lib.bmf_residual_plan, 100000, 20000) == (2, 313)     # 782 row blocks -> 2 groups of 313 tiles (625 tiles)
    # tiled: m_pad / 64 tiles; splits = min(ceil(1024 / tiles), max(stages / 8, 1)); per = ceil(stages / splits); splits = ceil(stages / per)
    assert plan(lib.bmf_residual_tiled_plan, 64, 64) == (1, 1)
    assert plan(lib.bmf_residual_tiled_plan, 64, 64 * 15) == (1, 15)
    assert plan(lib.bmf_residual_tiled_plan, 64, 64 * 17) == (2, 9)   # two splits, 9 + 8 stages
    assert plan(lib.bmf_residual_tiled_plan, 192, 64 * 23) == (2, 12)
    assert plan(lib.bmf_residual_tiled_plan, 384, 1024) == (2, 8)     # the shape of test_tiled_real_matrix_kernels: two full splits
    assert plan(lib.bmf_residual_tiled_plan, 64 * 2048, 64 * 64) == (1, 64)   # 2048 tiles fill the chip: one split
    assert plan(lib.bmf_residual_tiled_plan, 64 * 100, 64 * 1000) == (11, 91)  # ceil(1024 / 100) = 11 splits of 91 (the last 90)
    # bmf_mae_plan needs the compute-unit count, so only its argument checks run here
    assert lib.bmf_mae_plan(256, 64, None, C.byref(b)) == -1 and b"bmf_mae_plan: null pointer" in lib.bmf_last_error()
    for bad in ((0, 64), (255, 64), (256, 0), (256, 65), (-256, 64), (1 << 32, 64)):
        assert lib.bmf_mae_plan(bad[0], bad[1], C.byref(a), C.byref(b)) == -1 and b"bmf_mae_plan" in lib.bmf_last_error(), bad
    # bmf_xf_bits_i8_plan with an explicit compute-unit count is host arithmetic too: its arguments are checked as the launch checks them
    f, total, perm = (C.c_int32 * 8)(*([-7] * 8)), C.c_int64(-7), (C.c_uint16 * 512)(*([7] * 512))
    good = dict(rows_pad=1024, red_words=32, ncols=32, kp=64, cus=256)

    def i8_plan(plan=f, tot=total, pm=perm, **kw):
        a_ = dict(good, **kw)
        return lib.bmf_xf_bits_i8_plan(a_["rows_pad"], a_["red_words"], a_["ncols"], a_["kp"], a_["cus"], plan, C.byref(tot) if tot is not None else None, pm)

    assert i8_plan(plan=None) == -1 and b"bmf_xf_bits_i8_plan: null pointer" in lib.bmf_last_error()
    assert i8_plan(tot=None) == -1 and b"bmf_xf_bits_i8_plan: null pointer" in lib.bmf_last_error()
    for bad in (dict(rows_pad=0), dict(rows_pad=-512), dict(rows_pad=1000), dict(rows_pad=768), dict(red_words=0), dict(red_words=-16),
                dict(red_words=24), dict(red_words=1 << 19), dict(ncols=0), dict(ncols=16), dict(ncols=48), dict(ncols=96),
                dict(ncols=64, kp=32), dict(kp=48), dict(kp=128), dict(cus=-1), dict(cus=1), dict(cus=1 << 20),
                dict(rows_pad=1 << 40, red_words=(1 << 19) - 16)):
        assert i8_plan(**bad) == -1 and b"bmf_xf_bits_i8_plan" in lib.bmf_last_error(), bad
        assert list(f) == [-7] * 8 and total.value == -7 and list(perm) == [7] * 512, bad      # a refused call writes nothing
    assert i8_plan() == 0 and list(f) == [8, 8, 0, 4, 4, 2, 1, 256] and total.value == 32       # 4 tiles x 8 stages: 8 slices of one group
    assert sorted(perm) == list(range(8)) + [0xFFFF] * 504
    f[0] = -7
    assert i8_plan(pm=None) == 0 and f[0] == 8                                                  # the slice map is optional
    import objective_ref as R
    for m, n in ((1, 1), (130, 70), (128, 65606), (8192, 1083), (100000, 20000), (20, 33000)):
        assert plan(lib.bmf_residual_plan, m, n) == R.residual_plan(m, n)
    for mp, np_ in ((64, 64), (192, 64 * 23), (384, 1024), (6400, 64000)):
        assert plan(lib.bmf_residual_tiled_plan, mp, np_) == R.tiled_plan(mp, np_)


def test_no_cpu_fallback():
    """Without a GPU the product refuses to run instead of computing on the host."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import numpy as np
    from pybmf_amd.engine import BitMatrix
    from pybmf_amd.models import BinaryMFPenalty
    with pytest.raises(RuntimeError, match="no CPU path"):
        BitMatrix(np.zeros((8, 8), np.uint8), "cuda:0")
    with pytest.raises(RuntimeError, match="no CPU path"):
        BinaryMFPenalty(k=2, init_method="normal", seed=0).fit(np.eye(8, dtype=np.uint8), task="reconstruction",
                                                              show_logs=False, show_result=False, save_model=False)


def test_argument_checks_under_host_asan():
    """the C-ABI's argument-checking layer built with -fsanitize=address on the HOST side (CPU only) and driven
    through every entry point with arguments it must refuse before touching a GPU (tests/asan/abi_asan_driver.c)."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang"):
        pytest.skip("needs the ROCm clang for the sanitizer runtime")
    res = subprocess.run(["make", "-C", os.path.join(ROOT, "pybmf_amd", "csrc"), "-j", "8", "asan"], capture_output=True, text=True, timeout=1500)
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-1500:])
    assert "0 entry point(s) not refused" in res.stdout and "AddressSanitizer" not in res.stderr
