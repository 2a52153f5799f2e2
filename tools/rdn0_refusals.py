"""The refusals of oa_rdn0_set_data / oa_mc_run_rdn0 / oa_mc_run_rdn0_windowed provoked one by one through ctypes, one line each (entry,
status, oa_last_error): run it on two builds (ORPHICS_AMD_LIB selects the library) and diff the outputs when a change must not alter a
message.  Nothing is launched beyond plan creation, the filter / bin binding and one oa_rdn0_set_data."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orphics_amd import _lib, cosmology, lensing, maps  # noqa: E402
from orphics_amd.geometry import FlatGeometry  # noqa: E402

lib = _lib.load()
ok = _lib.check
V = ctypes.c_void_p


def dev(a):
    a = np.ascontiguousarray(a)
    p = V()
    ok(lib.oa_malloc(ctypes.byref(p), a.nbytes))
    ok(lib.oa_memcpy(p, a.ctypes.data_as(V), a.nbytes, 1, None))
    return p


def say(tag, rc):
    print("%-34s rc=%d  %s" % (tag, rc, lib.oa_last_error().decode() if rc else "(accepted)"), flush=True)


def plan_of(shape, res):
    g = FlatGeometry.from_res(shape, res)
    th, ml = cosmology.default_theory(), g.modlmap()
    beam, noise = maps.gauss_beam(ml, 1.5), np.full(shape, cosmology.white_noise_power(1.0))
    q = lensing.qest(shape, g, th, noise2d=noise, beam2d=beam, kmask=maps.mask_kspace(shape, g, lmin=300, lmax=2000),
                     kmask_K=maps.mask_kspace(shape, g, lmin=20, lmax=3000), unlensed_equals_lensed=True, dtype="f32")
    plan = V()
    ok(lib.oa_plan_create(shape[0], shape[1], _lib.OA_F32, ctypes.byref(plan)))
    ly, lx = g.laxes()
    ok(lib.oa_plan_set_laxes(plan, ly.ctypes.data_as(V), lx.ctypes.data_as(V)))
    return q, plan


buf = dev(np.zeros(1 << 16))                      # stands in for cs, window, n, S, C: every call below is refused before it reads them
entries = (("oa_mc_run_rdn0", lambda p, w=buf: lib.oa_mc_run_rdn0(p, 1, 0, 2, buf, buf, buf, buf, None)),
           ("oa_mc_run_rdn0_windowed", lambda p, w=buf: lib.oa_mc_run_rdn0_windowed(p, 1, 0, 2, buf, w, buf, buf, buf, None)))


def every(tag, plan):
    for name, f in entries:
        say(name + " " + tag, f(plan))


every("NULL plan", None)
say("oa_rdn0_set_data NULL", lib.oa_rdn0_set_data(None, None, None))
say("oa_mc_run_rdn0_windowed NULL window", entries[1][1](None, None))
qz, pz = plan_of((112, 154), 4.0)
every("chirp-z", pz)
say("oa_rdn0_set_data chirp-z", lib.oa_rdn0_set_data(pz, buf, None))
q, plan = plan_of((256, 256), 2.0)
say("oa_mc_run_rdn0_windowed NULL window", entries[1][1](plan, None))
every("no filters", plan)
say("oa_rdn0_set_data no filters", lib.oa_rdn0_set_data(plan, buf, None))
F = [dev(t.cpu().numpy()) for t in q._F["TT"]]
bind = lambda: ok(lib.oa_plan_set_filters(plan, F[0], F[1], F[2], q.leg_cols, q.kappa_cols, q.leg_rows, q.kappa_rows, -1))
bind()
every("no bins", plan)
import torch  # noqa: E402
edges = np.linspace(100, 2900, 12)
ids = q.eng.modl_digitize(torch.as_tensor(edges, device=q.eng.device), half=True)
ok(lib.oa_plan_set_bins(plan, dev(ids.cpu().numpy()), edges.size + 1, 1.0, None))
every("no data", plan)
kd = dev(np.zeros((256, q.eng.kp, 2), dtype=np.float32))
say("oa_rdn0_set_data", lib.oa_rdn0_set_data(plan, kd, None))
bind()
every("stale", plan)
# a 2^a 3^b 5^c plan whose filters span the whole plane: no band grid smaller than the map
qm, pm = plan_of((300, 360), 2.0)
Fm = [dev(t.cpu().numpy()) for t in qm._F["TT"]]
say("oa_plan_set_filters full plane", lib.oa_plan_set_filters(pm, Fm[0], Fm[1], Fm[2], 180, 181, 150, 150, -1))
say("oa_rdn0_set_data no band grid", lib.oa_rdn0_set_data(pm, buf, None))
idm = qm.eng.modl_digitize(torch.as_tensor(edges, device=qm.eng.device), half=True)
say("oa_plan_set_bins", lib.oa_plan_set_bins(pm, dev(idm.cpu().numpy()), edges.size + 1, 1.0, None))
every("no band grid", pm)
ok(lib.oa_stream_synchronize(None))
