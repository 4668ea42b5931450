"""Which kernels the library holds in both roundings of the band LU (namespaces lu_fma / lu_nofma, option "lu_fma"), read off the symbol
tables of the two library flavours: the kernels that hold the LU -- the column solve (tmx_k_column.hip) and the implicit column update of
the tracers (tmx_k_tracer_solve.hip) -- and no other.  The vertical kernels without an LU (tmx_k_vertical.hip) are compiled once, outside
any namespace, and their launchers are ordinary functions: a second copy of them would be the same instructions shipped twice."""
import os
import re
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernels without a band LU, by the start of their names (every instantiation and form), and their launchers
NO_LU_KERNELS = ("k_v_explicit", "k_v_tracers_explicit", "k_v_filter_tracers", "k_vi_terms_explicit")
NO_LU_LAUNCHERS = ("tmxk_v_explicit", "tmxk_vi_terms_explicit", "tmxk_v_filter_tracers", "tmxk_vi_tracers_explicit")
# kernels that hold it, and the launchers tmx_lu_select.hip dispatches
LU_KERNELS = ("k_vi_pair", "k_vi_group", "k_vi_tracers_rows")
LU_LAUNCHERS = ("tmxk_vi_fused", "tmxk_vi_tracers", "tmxk_vi_tracers_all")


def _functions(path):
    """[(namespace or "", function name)] of the library's demangled symbols"""
    out = subprocess.run(["nm", "-C", path], capture_output=True, text=True, check=True).stdout
    found = []
    for line in out.splitlines():
        m = re.match(r"[0-9a-f ]{16} \w (?:void )?(?:__device_stub__)?((?:\w+::)*)(\w+)[<(]", line)
        if m:
            found.append((m.group(1).rstrip(":"), m.group(2)))
    return found


@pytest.mark.parametrize("flavour", ["production", "experiments"])
def test_only_the_kernels_that_hold_the_band_lu_are_built_in_both_roundings(flavour):
    if not shutil.which("nm"):
        pytest.skip("no nm on this machine: the library's symbol table cannot be read")
    path = os.path.join(ROOT, "tempestmodel_amd", "libtempest_mi355x%s.so" % ("_exp" if flavour == "experiments" else ""))
    fns = _functions(path)
    spaces = {"lu_fma", "lu_nofma"}
    # the reading works: what holds the LU is there in both namespaces, kernels and launchers
    for name in LU_KERNELS + LU_LAUNCHERS:
        assert {ns for ns, fn in fns if fn == name} >= spaces, (name, "not in both namespaces")
    doubled = sorted({(ns, fn) for ns, fn in fns if ns in spaces and (fn.startswith(NO_LU_KERNELS) or fn in NO_LU_LAUNCHERS)})
    assert not doubled, "compiled in both roundings of the band LU without holding one: %s" % (doubled,)
    for start in NO_LU_KERNELS:
        assert any(ns == "" and fn.startswith(start) for ns, fn in fns), (start, "no kernel of that name outside the namespaces")
    for name in NO_LU_LAUNCHERS:
        assert ("", name) in fns, (name, "not an ordinary function")
    # every kernel in the namespaces is one of the column solve or the tracer solve
    inside = sorted({fn for ns, fn in fns if ns in spaces and fn.startswith("k_")})
    assert all(fn.startswith(("k_vi_pair", "k_vi_group", "k_vi_fused", "k_vi_back", "k_vi_assemble", "k_vi_solve", "k_vi_tracers_rows")) for fn in inside), inside
