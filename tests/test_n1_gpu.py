"""GPU: ``oa_n1_tt`` (orphics_amd/csrc/n1.hip) against the NumPy statement of tests/test_n1_cpu.py, its determinism, its refusals, and the
``Estimator`` / ``NlGenerator`` surface.  Pass condition of the sums: |S_gpu - S_ref| <= 1e-12 sum|term| (see test_n1_cpu.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import test_n1_cpu as st  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = st.TOL

# (Ny, Nx), band, modes: one L on each axis, one with negative ky and kx, one generic
CASES = {
    "32x32": ((32, 32), (5, 5), [(3, 0), (0, 4), (29, 28), (2, 7)]),                 # box 11 x 11: smaller than one tile
    "64x48": ((64, 48), (9, 7), [(5, 0), (0, 6), (57, 43), (11, 3)]),                # mixed-radix side, box 19 x 15: remainders on both axes
    "128x128": ((128, 128), (20, 20), [(7, 0), (0, 9), (120, 117), (13, 22)]),       # box 41 x 41, 2.8e6 pairs: several workgroups and the fold
    # box 3 x 601: a box row is two l1 tiles (> 512 modes) and five q chunks (> 128 modes) -- the paths no square box of this size reaches
    "32x4096": ((32, 4096), (1, 300), [(1, 0), (0, 37), (31, 4000), (2, 250)]),
}


@pytest.fixture(scope="module")
def engines():
    from orphics_amd.engine import Engine
    made = {}

    def get(shape, prec="f64", laxes=True):
        key = (shape, prec, laxes)
        if key not in made:
            e = Engine(shape[0], shape[1], prec)
            if laxes:
                res = 2.0 * np.pi / 180 / 60                      # make_case's axes (car: x decreases, except at 32 x 32)
                e.set_laxes(2 * np.pi * np.fft.fftfreq(shape[0], res), 2 * np.pi * np.fft.fftfreq(shape[1], res if shape[0] == 32 else -res))
            made[key] = e
        return made[key]
    return get


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (shape, band, modes) in CASES.items():
        case = st.make_case(*shape, *band, seed=shape[0] + shape[1], car=shape[0] != 32)
        out[name] = (case, modes, st.reference(case, modes))
    return out


def _planes(e, case):
    import torch
    return [torch.as_tensor(st.hc_plane(case[k], e.kp, fill=0.0), dtype=torch.float64, device=e.device) for k in ("wg", "wh", "cr", "cpp")]


def _run(e, case, modes):
    pl = _planes(e, case)
    return e.n1_tt(*pl, case["cols"], case["rows"], [m[0] for m in modes], [m[1] for m in modes]).cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_sums_against_the_statement(engines, cases, name):
    case, modes, (ref, scale) = cases[name]
    e = engines((case["Ny"], case["Nx"]))
    S = _run(e, case, modes)
    err = np.abs(S - ref) / scale
    print("n1 %s: S %s  |S - ref| / sum|term| %s" % (name, S, err))
    assert np.all(scale > 0) and np.abs(ref).max() > 1e-3 * scale.max()
    assert np.all(np.abs(S - ref) <= TOL * scale), err.max()
    # two identical calls: the same bits; the list cut into two calls: the same bits
    assert np.array_equal(S, _run(e, case, modes))
    assert np.array_equal(S, np.concatenate([_run(e, case, modes[:1]), _run(e, case, modes[1:])]))


def test_zero_modes_and_pool_release(engines, cases):
    case, modes, _ = cases["32x32"]
    e = engines((32, 32))
    S = _run(e, case, [(0, 0), (11, 0), (16, 16), modes[0]])        # L = 0: g = 0; |L| beyond twice the band: no pair
    assert np.all(S[:3] == 0.0) and S[3] != 0.0
    e.release_pools()
    assert np.array_equal(_run(e, case, [modes[0]]), S[3:])


def test_refusals_by_name_with_nothing_launched(engines, cases):
    import torch
    from orphics_amd import _lib
    case, modes, _ = cases["32x32"]
    lib = _lib.load()
    e = engines((32, 32))
    pl = _planes(e, case)
    SENT = -7.5
    out = torch.full((2,), SENT, dtype=torch.float64, device=e.device)
    Ly, Lx = np.array([3, 2], dtype=np.int32), np.array([0, 7], dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    tp = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(plan, planes, cols, rows, nL, ly=Ly, lx=Lx):
        rc = lib.oa_n1_tt(plan, *[tp(t) for t in planes], cols, rows, nL, vp(ly), vp(lx), tp(out), None)
        torch.cuda.synchronize()
        return rc, lib.oa_last_error().decode()
    e32 = engines((32, 32), "f32")
    bare = engines((32, 32), "f64", laxes=False)
    for args, word in [((e32.plan, pl, 6, 6, 2), "float64"),
                       ((bare.plan, pl, 6, 6, 2), "oa_plan_set_laxes"),
                       ((e.plan, pl, 6, 10, 2), "un-aliased"),
                       ((e.plan, pl, 10, 6, 2), "un-aliased"),
                       ((e.plan, pl, 6, 6, 0), "nL"),
                       ((e.plan, pl, 6, 6, 2, np.array([3, 32], dtype=np.int32), Lx), "outside"),
                       ((e.plan, pl, 6, 6, 2, Ly, np.array([-1, 7], dtype=np.int32)), "outside")]:
        rc, msg = call(*args)
        assert rc != 0 and msg.startswith("oa_n1_tt:") and word in msg, msg
        assert np.all(out.cpu().numpy() == SENT)
    rc, _ = call(e.plan, pl, 6, 6, 2)
    assert rc == 0 and np.all(out.cpu().numpy() != SENT)
    # the wrapper refuses on the host
    with pytest.raises(ValueError, match="float64"):
        e32.n1_tt(*pl, 6, 6, [3], [0])
    with pytest.raises(ValueError, match="un-aliased"):
        e.n1_tt(*pl, 6, 10, [3], [0])


@pytest.fixture(scope="module")
def nlgen256():
    from orphics_amd import cosmology
    from orphics_amd.geometry import FlatGeometry
    from orphics_amd.lensing import NlGenerator
    shape = (256, 256)
    geom = FlatGeometry.from_res(shape, 2.0)
    g = NlGenerator(shape, geom, cosmology.default_theory(), bin_edges=np.linspace(100, 3000, 6))
    g.updateNoise(1.5, 1.0, 1.4, 300, 2000, 300, 2000)              # the notebook filters
    return g


def test_estimator_surface(nlgen256):
    q = nlgen256.q
    rows, cols = q.n1_band()
    assert 4 * (rows - 1) < 256 and 4 * (cols - 1) < 256 and rows > 30
    modes = np.array([[5, 0], [0, 20], [250, 240], [30, 40]])
    S = q.n1_sums(modes)
    assert S.shape == (4,) and np.all(np.isfinite(S)) and np.all(S != 0)
    ly, lx = q.geom.laxes()
    L = np.hypot(ly[modes[:, 0]], lx[modes[:, 1]])
    AL = q._full(q.AL["TT"])[modes[:, 0], modes[:, 1]]
    want = (L * (L + 1) / 2) ** 2 * AL ** 2 * S / q.geom.area ** 2
    got = q.N1_kappa(modes)
    assert np.all(AL > 0) and np.allclose(got, want, rtol=1e-14, atol=0)
    assert np.allclose(q.N1_phi(modes), AL ** 2 * S / q.geom.area ** 2, rtol=1e-14, atol=0)
    # linear in C^phiphi; and S(L) = S(-L) for the isotropic filters
    # (1e-9 of the largest sum: rounding of sums whose terms cancel, far below any convention defect)
    assert np.abs(q.n1_sums(modes, clpp_half=3.0 * q.n1_clpp()) - 3.0 * S).max() <= 1e-9 * np.abs(S).max()
    assert np.abs(q.n1_sums((-modes) % 256) - S).max() <= 1e-9 * np.abs(S).max()
    # the estimator's run precision does not enter: the sums run on the float64 engine
    assert np.array_equal(q.astype("f32").n1_sums(modes), S)
    # a band too wide for the grid is refused by name
    import copy
    wide = copy.copy(q)
    wide.wg_tt = np.ones_like(q.wg_tt)
    with pytest.raises(ValueError, match="un-aliased"):
        wide.n1_sums(modes)


def test_getN1(nlgen256):
    cents, n1 = nlgen256.getN1("TT", per_bin=2)
    assert cents.shape == n1.shape == (5,) and np.all(np.isfinite(n1)) and np.any(n1 != 0)
    q32 = nlgen256.q.astype("f32")
    saved, nlgen256.q = nlgen256.q, q32
    try:
        _, n1_32 = nlgen256.getN1("TT", per_bin=2)
    finally:
        nlgen256.q = saved
    assert np.array_equal(np.sign(n1_32), np.sign(n1)) and np.array_equal(n1_32, n1)
    print("getN1 256^2 2': centers %s N1_kk %s" % (cents, n1))
    with pytest.raises(NotImplementedError, match="follow-up"):
        nlgen256.getN1("EE")
