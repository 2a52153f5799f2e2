"""CPU: the surface of the polarisation / MV N0 Monte Carlo that needs no GPU -- the three C-ABI entries are declared and bound, the
sample vector's spectrum list and labels, and the square root of the T, E, B covariance."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("oa_grf_mix_band", "oa_bin_power_multi", "oa_bin_power_multi_scratch_bytes", "oa_mc_run_mv")


def test_entries_are_declared_and_bound():
    from orphics_amd import _lib
    txt = open(os.path.join(ROOT, "include", "orphics_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in the header"
        assert name in _lib.SIGNATURES, name + " is not in _lib.SIGNATURES"
    # argument counts of the declarations and of the ctypes table agree
    for name in ENTRIES:
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert int(re.search(r"#define OA_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION >= 407


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("mv", [False, True])
def test_spectrum_list_and_labels(cross, mv):
    from orphics_amd import mc
    ests = ("TT", "TE", "EE", "EB", "TB")
    labels, pairs = mc.pol_spectrum_list(ests, cross=cross, mv=mv)
    n = len(ests)
    assert len(labels) == len(pairs) == n + (n * (n - 1) // 2 if cross else 0) + (1 if mv else 0)
    # autos first, in estimator order
    assert labels[:n] == [(x, x) for x in ests] and pairs[:n] == [(i, i) for i in range(n)]
    at = n
    if cross:                     # upper triangle, row by row
        want = [(i, j) for i in range(n) for j in range(i + 1, n)]
        assert pairs[at:at + len(want)] == want
        assert labels[at:at + len(want)] == [(ests[i], ests[j]) for i, j in want]
        assert labels[at] == ("TT", "TE") and labels[at + len(want) - 1] == ("EB", "TB")
        at += len(want)
    if mv:                        # the MV auto is last and names field index n
        assert labels[at] == ("MV", "MV") and pairs[at] == (n, n)
        at += 1
    assert at == len(labels)
    assert all(0 <= a <= n and 0 <= b <= n for a, b in pairs)
    assert mv or all(a < n and b < n for a, b in pairs)
    assert len(set(labels)) == len(labels)


def test_spectrum_list_of_one_estimator_and_bad_sets():
    from orphics_amd import mc
    assert mc.pol_spectrum_list(("EB",), cross=True, mv=False) == ([("EB", "EB")], [(0, 0)])
    assert mc.pol_spectrum_list(("EB", "TB"), cross=True, mv=True) == ([("EB", "EB"), ("TB", "TB"), ("EB", "TB"), ("MV", "MV")],
                                                                      [(0, 0), (1, 1), (0, 1), (2, 2)])
    for bad in ((), ("TT", "TT"), ("TT", "TE", "EE", "EB", "TB", "ET", "BE")):
        with pytest.raises(ValueError):
            mc.pol_spectrum_list(bad)


def test_covariance_square_root_reproduces_the_powers():
    from orphics_amd import mc
    rng = np.random.default_rng(3)
    shape = (16, 9)
    TT = rng.uniform(0.5, 2.0, shape)
    EE = rng.uniform(0.5, 2.0, shape)
    BB = rng.uniform(0.0, 1.0, shape)
    TE = rng.uniform(-0.6, 0.6, shape) * np.sqrt(TT * EE)
    # modes without temperature power (a masked monopole, a filtered band): TE vanishes with TT there, EE need not
    TT[0, 0] = 0.0; TE[0, 0] = 0.0
    TT[5, 3:6] = 0.0; TE[5, 3:6] = 0.0
    BB[2, 2] = 0.0
    with np.errstate(all="raise"):            # the safe division divides nowhere by zero
        a, b, c, d = mc.teb_covsqrt(dict(TT=TT, EE=EE, BB=BB, TE=TE))
    for x in (a, b, c, d):
        assert x.shape == shape and np.all(np.isfinite(x))
    assert np.all(b[TT == 0] == 0)
    np.testing.assert_allclose(a * a, TT, rtol=1e-14, atol=0)
    np.testing.assert_allclose(a * b, TE, rtol=1e-14, atol=1e-300)
    np.testing.assert_allclose(b * b + c * c, EE, rtol=1e-13, atol=0)
    np.testing.assert_allclose(d * d, BB, rtol=1e-14, atol=0)
    assert np.all(a >= 0) and np.all(c >= 0) and np.all(d >= 0)
