"""CPU: the host-only surface of the pol / MV RDN0 on the band grid of sides 2^a 3^b 5^c -- the header's declaration and contract of
``oa_grf_mix_band_inner_triples``, the band-grid paragraph of ``oa_rdn0_set_data_mv`` / ``oa_mc_run_rdn0_mv``, the ctypes signature, the ABI
version and the docstring of ``mc.RDN0MonteCarloPol(one_call="band")``."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "orphics_amd.h")).read()


def test_header_declares_the_draw_and_the_binding_holds_it():
    from orphics_amd import _lib
    flat = " ".join(header().split())
    want = ("int oa_grf_mix_band_inner_triples(oa_plan* p, uint64_t seed, uint64_t stream_id0, int ntriples, const void* const* covsqrt_hc, "
            "double scale, void* const* hc_out, int my, long out_pitch, int width, int rband, void* stream);")
    assert want in flat
    sig = _lib.SIGNATURES["oa_grf_mix_band_inner_triples"]
    assert sig[0] is _lib.c_int and len(sig[1]) == 12
    # ntriples sits where the single-triple entry has ncomp: the argument types are the same
    assert list(sig[1]) == list(_lib.SIGNATURES["oa_grf_mix_band_inner"][1])
    doc = flat[flat.index("ntriples (1 or 2) T, E, B triples of oa_grf_mix_band_inner"):flat.index(want)]
    for piece in ("bit for bit", "stream_id0 + 3 z", "once for its triple", "nothing outside the band", "ntriples outside 1..2"):
        assert piece in doc, piece


def test_abi_versions_match_and_moved():
    from orphics_amd import _lib
    ver = int(re.search(r"#define\s+OA_ABI_VERSION\s+(\d+)", header()).group(1))
    assert ver == _lib.ABI_VERSION > 414


def test_header_band_grid_paragraph_names_both_bindings():
    flat = " ".join(header().split())
    start = flat.index("REALISATION-DEPENDENT N0 of an estimator SET")
    par = flat[start:flat.index("int oa_rdn0_set_data_mv(", start)]
    assert "ON A BAND GRID (2^a 3^b 5^c plans)" in par
    band = par[par.index("ON A BAND GRID (2^a 3^b 5^c plans)"):]
    for piece in ("oa_qe_band_bind", "oa_mc_mv_band_bind", "in this order", "oa_grf_mix_band_inner_triples", "nspec_max", "stale",
                  "mc.RDN0MonteCarloPol", "one_call=False", "Nyquist column is never visited", "oa_mc_run_rdn0_mv_windowed is NOT on the band grid"):
        assert piece in band, piece
    assert band.index("oa_qe_band_bind") < band.index("oa_mc_mv_band_bind") < band.index("then oa_rdn0_set_data_mv")
    assert "no band grid yet" not in flat and "band grid of sides 2^a 3^b 5^c yet" not in flat


def test_docstring_describes_band_and_keeps_the_older_sentences():
    from orphics_amd import mc
    doc = " ".join(mc.RDN0MonteCarloPol.__doc__.split())
    keep = "band-grid sides (2^a 3^b 5^c) run the host loop for now"
    for piece in (keep, "one_call=False", "There is no window argument to the constructor", "set_window", "ALREADY apodised",
                  "oa_mc_run_rdn0_mv_windowed", "``one_call=None`` (default): the one call on power-of-two sides, the host loop elsewhere"):
        assert piece in doc, piece
    band = doc[doc.index('``one_call="band"``'):]
    assert doc.index(keep) < doc.index('``one_call="band"``')
    for piece in ("on power-of-two sides it behaves as ``True``", "qest.one_call_pol(estimators, ext_norm=True)", "qest._pol_bands(estimators, True)",
                  "oa_qe_band_bind", "oa_mc_mv_band_bind", "oa_rdn0_set_data_mv", "oa_grf_mix_band_inner_triples", "``OrphicsAmdError``",
                  "``ValueError``", ":meth:`set_window` raises"):
        assert piece in band, piece


def test_constructor_signature_is_unchanged_and_bad_strings_are_refused_first():
    from orphics_amd import mc
    sig = inspect.signature(mc.RDN0MonteCarloPol.__init__)
    assert list(sig.parameters)[1:] == ["qest", "data", "total_power_half", "bin_edges", "estimators", "cross", "mv", "comm", "base_seed", "one_call",
                                        "qu", "iau"]
    assert sig.parameters["one_call"].default is None
    try:                                   # refused before anything touches the estimator (None here) or a device
        mc.RDN0MonteCarloPol(None, None, None, None, one_call="bands")
    except ValueError as ex:
        assert "band" in str(ex)
    else:
        raise AssertionError("one_call=\"bands\" was accepted")
    assert hasattr(mc.RDN0MonteCarloPol, "set_window") and "grf_mix_band_inner_triples" in dir(__import__("orphics_amd.engine", fromlist=["Engine"]).Engine)
