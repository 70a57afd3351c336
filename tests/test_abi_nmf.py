"""The coordinate-descent NMF entry points of the C ABI (bmf_nmf_cd_sweep, bmf_nmf_cd_iterate): the ctypes mirror of bmf_nmf_state has
the C layout, and bad arguments are refused with an error code and a message before anything touches a GPU (no GPU needed)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bmf_hip.h")


def test_state_layout_matches_c(tmp_path):
    from pybmf_amd import _lib as L
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu\\n", sizeof(bmf_nmf_state),'
                   'offsetof(bmf_nmf_state, m_pad), offsetof(bmf_nmf_state, Xtiled), offsetof(bmf_nmf_state, partU),'
                   'offsetof(bmf_nmf_state, log));return 0;}\n' % HEADER)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(L.NmfState), L.NmfState.m_pad.offset, L.NmfState.Xtiled.offset, L.NmfState.partU.offset, L.NmfState.log.offset]
    assert L.lib.bmf_struct_bytes(8) == C.sizeof(L.NmfState)


def sweep(lib, **over):
    """bmf_nmf_cd_sweep with plausible arguments (fake, aligned, never dereferenced pointers), some of them replaced."""
    p = C.c_void_p(4096)
    a = dict(F64=p, F=p, rows_pad=256, rows=200, k=5, kp=32, num=p, slab_stride=256 * 32, splits=2, G64=p, blockmax=p, viol=p)
    a.update(over)
    return lib.bmf_nmf_cd_sweep(a["F64"], a["F"], a["rows_pad"], a["rows"], a["k"], a["kp"], a["num"], a["slab_stride"], a["splits"], a["G64"],
                                a["blockmax"], a["viol"], None)


def test_sweep_refuses_bad_arguments_without_a_gpu():
    from pybmf_amd import _lib as L
    lib = L.lib
    for name in ("F64", "F", "num", "G64", "blockmax", "viol"):
        assert sweep(lib, **{name: None}) == -1 and b"null pointer" in lib.bmf_last_error(), name
    for over, text in ((dict(rows_pad=200), b"multiple of 128"), (dict(rows_pad=0), b"multiple of 128"), (dict(rows=0), b"rows"),
                       (dict(rows=257), b"rows"), (dict(kp=48), b"kp"), (dict(k=0), b"k="), (dict(k=33), b"k="), (dict(k=65, kp=64), b"k="),
                       (dict(splits=0), b"slab"), (dict(slab_stride=256 * 32 - 4), b"slab"), (dict(slab_stride=256 * 32 + 2), b"slab"),
                       (dict(F64=C.c_void_p(4104)), b"aligned"), (dict(F=C.c_void_p(4100)), b"aligned"), (dict(num=C.c_void_p(4100)), b"aligned")):
        assert sweep(lib, **over) == -1, over
        assert text in lib.bmf_last_error(), (over, lib.bmf_last_error())


def plausible_state(L):
    st = L.NmfState()
    st.struct_bytes = C.sizeof(L.NmfState)
    st.m, st.n, st.k, st.kp = 700, 450, 5, 32
    st.splits_xv = st.splits_xtu = st.gram_blocks = 2
    st.log_rows = 8
    st.m_pad, st.n_pad = 1024, 512
    for name, _ in L.NmfState._fields_:
        if getattr(L.NmfState, name).size == C.sizeof(C.c_void_p) and name not in ("m_pad", "n_pad"):
            setattr(st, name, 4096)
    return st


def test_iterate_refuses_bad_states_without_a_gpu():
    from pybmf_amd import _lib as L
    lib = L.lib
    assert lib.bmf_nmf_cd_iterate(None, 0, None) == -1 and b"null state" in lib.bmf_last_error()
    st = L.NmfState()
    assert lib.bmf_nmf_cd_iterate(C.byref(st), 0, None) == -1 and b"struct_bytes" in lib.bmf_last_error()
    for change, text in ((dict(Vpanel=None), b"null pointer"), (dict(log=None), b"null pointer"), (dict(partU=None), b"null pointer"),
                         (dict(m_pad=1000), b"512"), (dict(n_pad=0), b"512"), (dict(m=0), b"out of range"), (dict(n=513), b"out of range"),
                         (dict(kp=16), b"kp"), (dict(k=33), b"kp"), (dict(k=0), b"kp"), (dict(splits_xv=0), b"splits"),
                         (dict(gram_blocks=0), b"splits"), (dict(log_rows=0), b"log_rows")):
        st = plausible_state(L)
        for name, value in change.items():
            setattr(st, name, value)
        assert lib.bmf_nmf_cd_iterate(C.byref(st), 0, None) == -1, change
        assert text in lib.bmf_last_error(), (change, lib.bmf_last_error())
    assert lib.bmf_nmf_cd_iterate(C.byref(plausible_state(L)), -1, None) == -1 and b"it >= 0" in lib.bmf_last_error()
