"""The build-time names of the kernel sources are a closed list.

Every name that a preprocessor conditional of tempestmodel_amd/csrc tests is either a named tuning number (one number, no second
body of code), a diagnostic of the kernels as they are, or one of the library's flavours.  An A/B switch that has been measured is
resolved and its losing side archived under tools/experiments/ (kernel_build_switches.patch), not left in the source.  Needs no
compiler and no library."""
import os, re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tempestmodel_amd", "csrc")

TUNING = {"KT_H", "KT_VE", "KT_VC", "TMX_H_MINWG", "TMX_HV_MINWG", "TMX_DSS_MINWG", "TMX_HW_WAVES_PER_EU", "TMX_RING_DEPTH", "TMX_GRP_PF",
          "TMX_EXPECT_T"}      # (one conditional on TMX_EXPECT_T guards the three numbers TMX_EXPECT_T / _W / _R)
DIAGNOSTICS = {"TMX_VI_TIMING", "TMX_PAIR_TIMING", "TMX_H_TIMING"}
FLAVOURS = {"TMX_EXP", "TMX_EXPERIMENTS", "TMX_LU_NOFMA", "__HIPCC__", "TMX_REFMATH_H"}
# two switches whose removal changed the compiler's output for a kernel (profiles/kernel_build_switches.md): they stay as they were
KEPT_FOR_THE_DEVICE_CODE = {"TMX_H_BURST", "TMX_DSS_LPT"}
ALLOWED = TUNING | DIAGNOSTICS | FLAVOURS | KEPT_FOR_THE_DEVICE_CODE


def conditional_names():
    """name -> files, for every identifier in the condition of an #if / #ifdef / #ifndef / #elif under csrc"""
    found = {}
    for name in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, name)
        if not os.path.isfile(path): continue
        text = open(path, errors="replace").read().replace("\\\n", " ")
        for m in re.finditer(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b([^\n]*)", text, flags=re.M):
            cond = re.sub(r"//.*|/\*.*?\*/", "", m.group(1))
            for ident in re.findall(r"[A-Za-z_]\w*", cond):
                if ident != "defined": found.setdefault(ident, set()).add(name)
    return found


def test_build_time_names_are_the_listed_ones():
    found = conditional_names()
    new = {n: sorted(f) for n, f in found.items() if n not in ALLOWED}
    gone = sorted(ALLOWED - set(found))
    assert not new and not gone, (
        "preprocessor conditionals of tempestmodel_amd/csrc test names outside the list: %s; listed names no conditional tests: %s.  "
        "The list is the table 'Build-time names' in DESIGN.md (section 5): a measured A/B switch is resolved and archived under "
        "tools/experiments/, a new tuning number or diagnostic is added to that table and to this test." % (new, gone))
