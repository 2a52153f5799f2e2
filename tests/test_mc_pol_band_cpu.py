"""CPU: the surface of the band-grid polarisation / MV N0 Monte Carlo that needs no GPU -- the two new C-ABI entries (the inner-layout
leg-band draw and the Monte-Carlo set-up entry) are declared in the header and bound in the ctypes table with the same argument counts,
at an ABI version that has them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("oa_grf_mix_band_inner", "oa_mc_mv_band_bind")


def header():
    txt = open(os.path.join(ROOT, "include", "orphics_amd.h")).read()
    return txt, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_entries_are_declared_and_bound():
    from orphics_amd import _lib
    _, code = header()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in the header"
        assert name in _lib.SIGNATURES, name + " is not in _lib.SIGNATURES"


def test_argument_counts_agree():
    from orphics_amd import _lib
    _, code = header()
    want = {"oa_grf_mix_band_inner": 12, "oa_mc_mv_band_bind": 7}
    for name in ENTRIES:
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == want[name], name


def test_abi_version_has_them():
    from orphics_amd import _lib
    txt, _ = header()
    assert int(re.search(r"#define OA_ABI_VERSION (\d+)", txt).group(1)) >= 408
    assert _lib.ABI_VERSION >= 408
