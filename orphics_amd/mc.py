"""Monte-Carlo driver: Gaussian realisations -> TT reconstruction -> bandpowers,
sharded over GPUs with the reference's task split and ONE all-reduce at the end.

This is the north-star loop of tutorials/tt_verification.ipynb cell 4 /
SURVEY.md section 3.4 for the Gaussian (N0 / mean-field) case: every realisation
is independent, so ranks never talk until ``Statistics.allreduce`` time
(stats.py:1184-1232): n (int64), sum (d,), cross (d,d) and, optionally, the
mean-field stack (Ny, kp, 2) are summed over ranks with RCCL (gloo in CPU tests).
"""
import numpy as np

from . import mpi as _mpi
from .stats import Statistics


def _torch():
    import torch
    return torch


def allreduce_tensors(tensors, comm):
    """SUM all-reduce of device (or CPU) tensors in place over a TorchComm; no-op
    for a single rank / fake comm.  One collective per tensor, issued once per run."""
    if comm is None or comm.Get_size() == 1 or not hasattr(comm, "dist"):
        return tensors
    for t in tensors:
        comm.dist.all_reduce(t, op=comm.dist.ReduceOp.SUM, group=comm.group)
    return tensors


def _blocks(sims):
    """The non-empty list of indices ``sims`` cut where it stops being consecutive: [(lo, hi), ...], each block lo .. hi - 1."""
    out, lo = [], sims[0]
    for prev, i in zip(sims, sims[1:] + [None]):
        if i != prev + 1:
            out.append((lo, prev + 1))
            lo = i
    return out


def _run_sharded(driver, nsims, **kw):
    """Every driver's ``run``: this rank's share of ``nsims`` (mpi.mpi_distribute) through ``run_local``, ONE all-reduce, the Statistics."""
    comm = driver.comm
    _, tasks = _mpi.mpi_distribute(nsims, comm.Get_size(), allow_empty=True)
    driver.run_local(tasks[comm.Get_rank()], **kw)
    driver.acc.allreduce()
    return driver.acc


class GaussianN0MonteCarlo(object):
    """N0 bias / mean-field Monte Carlo on Gaussian maps with total power
    C_l^TT B_l^2 + N_l, generated on the device in harmonic space
    (MapGen semantics, maps.py:1576-1587, with the Philox stream (base_seed, sim index))."""

    def __init__(self, qest, total_power_half, bin_edges, comm=None, base_seed=1234, mean_field=False, streams=1, window=None,
                 one_call=None):
        """qest: lensing.Estimator; total_power_half: (Ny, Nx/2+1) host array of the
        observed-map power (C B^2 + N); bin_edges: kappa bandpower edges.
        window: (Ny, Nx) real-space apodisation (``maps.get_taper(shape, ...)[0]``) applied to every realisation before
        its transform, as the reference's analysis flow does (maps.py:1350-1361, 1873-1878): realisations are then drawn
        over the full plane and go through C2R -> x window -> R2C (``oa_mc_run_windowed``), and the mean-field stack no
        longer averages to zero.  ``window_moments`` = (mean w^2, mean w^4): bandpowers of kappa_hat (quadratic in the
        map) carry a factor mean(w^4) that the caller divides out (``debiased_mean``).
        streams > 1: this rank's simulations are split into that many contiguous blocks, each issued on its own HIP
        stream through a forked estimator handle (private plan and accumulators, summed at the end): the small
        latency-bound launches of independent realisations overlap.
        one_call (with a window): None (default) = ``oa_mc_run_windowed`` on power-of-two sides, a refusal elsewhere.
        ``one_call=True`` opts in to that call on sides 2^a 3^b 5^c as well: it runs on the estimator's band grid
        (``qest.one_call()``) and raises where there is none (chirp-z sides, unbounded filters, a band grid not smaller than
        the map).  ``one_call=False`` runs a host loop of the existing entries on any side, with the same seeds and
        Philox stream ids, on ONE HIP stream (``streams`` is not used there): ``Engine.grf_hc`` -> ``Engine.irfft`` -> x window -> ``Estimator.tt_moments`` (+ ``reconstruct_tt_from_map``
        into the mean-field stack); where the estimator has no one-call path at all, the modular reconstruction,
        ``Engine.bin_power`` and ``Statistics.add``."""
        torch = _torch()
        self.streams = max(1, int(streams))
        self.q = qest
        self.eng = qest.eng
        self.comm = comm if comm is not None else _mpi.get_world()
        self.base_seed = int(base_seed)
        self.mean_field = mean_field
        e = self.eng
        geom = qest.geom
        # unnormalised DFT of a unit-pixel-variance white map has |k|^2 = Npix; power p -> k = sqrt(p Npix^2/area) w
        amp = np.sqrt(np.asarray(total_power_half, dtype=np.float64) * float(e.npix) ** 2 / geom.area)
        self.cs = qest._hcreal(e, amp)
        self.edges = np.asarray(bin_edges, dtype=np.float64)
        self.ids = e.modl_digitize(torch.as_tensor(self.edges, device=e.device), half=True)
        self.nids = self.edges.size + 1
        self.d = self.nids - 2
        self.norm = geom.area / float(e.npix) ** 2
        # device-resident ensemble accumulators: (n, sum, cross) of the bandpower vectors and the mean-field stack
        self.acc = Statistics(comm=self.comm if hasattr(self.comm, "dist") else None, device=e.device)
        qest.bind_bins(self.ids, self.nids, self.norm)
        self.window = None
        self.window_moments = (1.0, 1.0)
        self.one_call = None if one_call is None else bool(one_call)
        if window is not None and not e.pow2 and self.one_call is None:
            from ._lib import OrphicsAmdError
            raise OrphicsAmdError("GaussianN0MonteCarlo: a window needs power-of-two map sides (oa_mc_run_windowed); %dx%d runs "
                                  "oa_mc_run on its band grid without a window only by default -- construct the driver with one_call=True "
                                  "(oa_mc_run_windowed on the band grid of sides 2^a 3^b 5^c) or one_call=False (host loop of the "
                                  "existing entries, any side)" % (e.ny, e.nx))
        if window is not None and not e.pow2 and self.one_call and not qest.one_call():
            from ._lib import OrphicsAmdError
            raise OrphicsAmdError("GaussianN0MonteCarlo: no one-call path on this %d x %d geometry (chirp-z sides, unbounded filters or a "
                                  "band grid not smaller than the map): construct the driver with one_call=False" % (e.ny, e.nx))
        self._host = None
        if window is not None:
            w = np.asarray(window, dtype=np.float64)
            if w.shape != (e.ny, e.nx):
                raise ValueError("window must be a (Ny, Nx) real-space array")
            self.window = e.to_real(w)
            self.window_moments = (float(np.mean(w ** 2)), float(np.mean(w ** 4)))

    def run_local(self, sims):
        """Process the given global sim indices on this rank's GPU: every contiguous block of indices is ONE
        ``oa_mc_run`` call (GRF -> TT estimator -> bandpowers -> moments [-> mean-field stack], no host work per sim)."""
        from ._lib import check
        from .engine import _ptr, _stream
        sims = [int(i) for i in sims]
        if not sims:
            return self
        q = self.q
        if self.window is not None and self.one_call is False:
            return self._run_host(sims)
        # (re)bind THIS driver's bins: another driver -- or a direct bind_bins call -- may have given the shared estimator
        # other edges since __init__, and the accumulators below are sized for self.d
        q.bind_bins(self.ids, self.nids, self.norm)
        e = q._bind_bins()
        n, S, C = self.acc.device_moments("n0", self.d)
        # kappa_hat vanishes outside its active region: the stack declares it, the all-reduce moves only that region
        sup = (q.kappa_rows, q.kappa_cols) if (q.kappa_cols and q.kappa_rows) else None
        mf = self.acc.device_stack("mf", (e.ny, e.kp, 2), support=sup) if self.mean_field else None
        blocks = _blocks(sims)
        # (with the mean-field stack the one-stream loop measured faster -- 16.0k vs 14.1k sims/s at 4096^2 -- so the
        # lanes are used for the bandpower moments only)
        if self.window is not None and self.streams > 1 and len(sims) >= 4 * self.streams:
            # windowed realisations are a chain of ~10 launches, half of them latency-bound (draw, leg kernel, row stage,
            # divergence + binning): independent realisations on several streams overlap them with the bandwidth-bound passes
            self._run_blocks_on_streams(blocks, n, S, C, mf)
        elif self.window is not None:
            for lo, hi in blocks:
                check(e.lib.oa_mc_run_windowed(e.plan, self.base_seed, lo, hi, _ptr(self.cs), _ptr(self.window), _ptr(n), _ptr(S), _ptr(C),
                                               _ptr(mf), _stream()))
        elif self.streams > 1 and len(sims) >= 4 * self.streams and not self.mean_field:
            self._run_blocks_on_streams(blocks, n, S, C, mf)
        else:
            for lo, hi in blocks:
                check(e.lib.oa_mc_run(e.plan, self.base_seed, lo, hi, _ptr(self.cs), _ptr(n), _ptr(S), _ptr(C), _ptr(mf), _stream()))
        self.acc.note_samples("n0", len(sims))
        if self.mean_field:
            self.acc.note_stacked("mf", len(sims))
        return self

    def _run_host(self, sims):
        """The windowed realisations ``sims`` through the existing entries, one by one (``one_call=False``): the full-plane draw of
        ``oa_mc_run_windowed`` (same seed and stream), ``Engine.irfft``, x window, then ``tt_moments`` -- or, where the estimator has no
        one-call path, the modular reconstruction, ``Engine.bin_power`` over kappa's band and ``Statistics.add``."""
        torch = _torch()
        q, e = self.q, self.eng
        sup = (q.kappa_rows, q.kappa_cols) if (q.kappa_cols and q.kappa_rows) else None
        mf = self.acc.device_stack("mf", (e.ny, e.kp, 2), support=sup) if self.mean_field else None
        fused = q.one_call()
        if self._host is None:
            cnt = None
            if not fused:     # data-independent mode counts per bin over the whole half plane
                zero = e.hc()
                cnt = e.bin_power(zero, zero, self.norm, self.ids, self.nids, herm=True)[1][1:-1].double()
            self._host = (e.hc(), e.real(), q.new_output(), cnt)
        draw, tmap, out, cnt = self._host
        if fused:
            q.bind_bins(self.ids, self.nids, self.norm)
            n, S, C = self.acc.device_moments("n0", self.d)
        for i in sims:
            e.grf_hc(self.base_seed, i, self.cs, out=draw)
            e.irfft(draw, out=tmap)
            tmap.mul_(self.window)
            kap = None
            if fused:
                q.tt_moments(tmap, n, S, C)
            else:
                kap = q.reconstruct_tt_from_map(tmap, out=out)
                s, _ = e.bin_power(kap, kap, self.norm, self.ids, self.nids, herm=True, active_cols=q.kappa_cols, active_rows=q.kappa_rows)
                self.acc.add("n0", s[1:-1] / cnt)
            if mf is not None:
                if kap is None:
                    kap = q.reconstruct_tt_from_map(tmap, out=out)
                mf += torch.view_as_real(kap).to(torch.float64)
        if fused:
            self.acc.note_samples("n0", len(sims))
        if self.mean_field:
            self.acc.note_stacked("mf", len(sims))
        return self

    def _run_blocks_on_streams(self, blocks, n, S, C, mf):
        """The blocks cut into ``self.streams`` pieces of (nearly) equal size; piece j runs on stream j with its own
        estimator handle and accumulators, which are added to (n, S, C, mf) in stream order at the end."""
        torch = _torch()
        from ._lib import check
        from .engine import _ptr
        K = self.streams
        if getattr(self, "_lanes", None) is None:
            lanes = []
            for j in range(K):
                qj = self.q if j == 0 else self.q.fork()
                qj.bind_bins(self.ids, self.nids, self.norm)
                own = None
                if j:     # private accumulators of this lane, allocated once and kept zero between calls
                    own = [torch.zeros_like(n), torch.zeros_like(S), torch.zeros_like(C), torch.zeros_like(mf) if mf is not None else None]
                lanes.append((qj, torch.cuda.Stream() if j else None, own))
            self._lanes = lanes
        sims = [i for lo, hi in blocks for i in range(lo, hi)]
        per = (len(sims) + K - 1) // K
        cur = torch.cuda.current_stream()
        parts = []
        for j, (qj, st, own) in enumerate(self._lanes):
            mine = sims[j * per:(j + 1) * per]
            if not mine:
                continue
            if j == 0:
                nj, Sj, Cj, mfj, stream = n, S, C, mf, cur
            else:
                nj, Sj, Cj, mfj = own
                stream = st
                stream.wait_stream(cur)
            with torch.cuda.stream(stream):
                qj.bind_bins(self.ids, self.nids, self.norm)
                ej = qj._bind_bins()
                for lo, hi in _blocks(mine):
                    if self.window is not None:
                        check(ej.lib.oa_mc_run_windowed(ej.plan, self.base_seed, lo, hi, _ptr(self.cs), _ptr(self.window), _ptr(nj),
                                                        _ptr(Sj), _ptr(Cj), _ptr(mfj), stream.cuda_stream))
                    else:
                        check(ej.lib.oa_mc_run(ej.plan, self.base_seed, lo, hi, _ptr(self.cs), _ptr(nj), _ptr(Sj), _ptr(Cj),
                                               _ptr(mfj), stream.cuda_stream))
            if j:
                parts.append((stream, nj, Sj, Cj, mfj))
        for stream, nj, Sj, Cj, mfj in parts:
            cur.wait_stream(stream)
            n += nj; S += Sj; C += Cj
            nj.zero_(); Sj.zero_(); Cj.zero_()
            if mf is not None:
                mf += mfj
                mfj.zero_()

    def run(self, nsims):
        """Shard ``nsims`` with mpi.mpi_distribute (mpi.py:78-91), run, reduce once; returns the reduced
        :class:`Statistics` (label 'n0' = kappa auto bandpowers, stack 'mf' = interleaved (re, im) sum of the
        kappa_hat DFTs if mean_field; ``stack_sum('mf', on_device=True)`` keeps it on the GPU)."""
        return _run_sharded(self, nsims)

    def debiased_mean(self):
        """mean kappa auto bandpowers of the (reduced) run divided by mean(w^4) of the window (1 without one)."""
        return self.acc.mean("n0") / self.window_moments[1]

    @property
    def centers(self):
        return (self.edges[1:] + self.edges[:-1]) / 2.


def pol_spectrum_list(estimators, cross=True, mv=True):
    """The sample vector of :class:`GaussianN0MonteCarloPol`: (labels, pairs).  Autos in estimator order, then -- ``cross`` -- the
    upper-triangle crosses row by row, then -- ``mv`` -- the auto of the MV combination.  A label is the pair of names, e.g.
    ("TT", "TT"), ("TT", "EB"), ("MV", "MV"); a pair holds the field indices ``oa_bin_power_multi`` takes (estimator e = field e, the
    MV combination = field ``len(estimators)``)."""
    ests = tuple(estimators)
    n = len(ests)
    if not 1 <= n <= 6 or len(set(ests)) != n:
        raise ValueError("1 to 6 distinct estimators, got %r" % (ests,))
    labels = [(x, x) for x in ests]
    pairs = [(i, i) for i in range(n)]
    if cross:
        for i in range(n):
            for j in range(i + 1, n):
                labels.append((ests[i], ests[j]))
                pairs.append((i, j))
    if mv:
        labels.append(("MV", "MV"))
        pairs.append((n, n))
    return labels, pairs


def teb_covsqrt(total_power):
    """Lower-triangular square root of the observed T, E, B covariance per mode: total_power = dict(TT, EE, BB, TE) of equally shaped
    arrays; returns (a, b, c, d) with T = a w0, E = b w0 + c w1, B = d w2 for unit white fields w: a = sqrt(TT), b = TE / a (0 where
    TT = 0), c = sqrt(EE - b^2), d = sqrt(BB), so that a^2 = TT, a b = TE, b^2 + c^2 = EE, d^2 = BB."""
    TT, EE, BB, TE = (np.asarray(total_power[k], dtype=np.float64) for k in ("TT", "EE", "BB", "TE"))
    a = np.sqrt(TT)
    b = np.zeros_like(a)
    np.divide(TE, a, out=b, where=a > 0)
    c = np.sqrt(np.maximum(EE - b ** 2, 0.0))
    d = np.sqrt(BB)
    return a, b, c, d


def _windowed_teb(e, base_seed, cs, rot, window, draw, maps, stream_id0):
    """The windowed T, E, B triple of Philox streams ``stream_id0 .. stream_id0 + 2`` through the existing entries (the host loop of the
    windowed pol drivers and the reference of their one calls): T, E, B -> T, Q, U in the draw's pass (``Engine.grf_mix(rot=(c, -s))`` on
    the full planes ``draw``), x window in real space (``Engine.irfft(window=...)`` into the real planes ``maps``), ``Engine.rfft`` back
    into ``draw``, then Q, U -> E, B (``Engine.rot2``): the window multiplies Q and U.  ``rot`` = (c, s, -s).  Returns (kT, kE, kB)."""
    c, s_, ms = rot
    e.grf_mix(base_seed, cs, rot=(c, ms), out=draw, stream_id0=int(stream_id0))
    for j in range(3):
        if e.pow2 or e.mixed:
            e.irfft(draw[j], out=maps[j], window=window)
        else:
            e.irfft(draw[j], out=maps[j])
            maps[j].mul_(window)
        e.rfft(maps[j], out=draw[j])
    kE, kB = e.rot2(c, s_, draw[1], draw[2])
    return draw[0], kE, kB


class GaussianN0MonteCarloPol(object):
    """N0 Monte Carlo of an estimator set (TT, TE, EE, EB, TB) and its MV combination on Gaussian T, E, B fields with the observed
    total powers: per realisation the bandpowers of every estimator's auto spectrum, of the N0 cross spectra N0^{ab} and of the MV
    kappa_hat's auto spectrum are ONE sample vector (``spectra`` = its blocks, ``len(bin_edges) - 1`` bins each), accumulated as
    (n, sum, cross) under the label "n0".  The MV auto is the variance of the kappa_hat that ``reconstruct_mv_hc`` returns -- which
    ``Estimator.Nlkk["MV"]`` (diagonal approximation) is not.

    Realisation i draws T, E, B with the Philox streams (base_seed, 3 i .. 3 i + 2), mixed by the lower-triangular square root of the
    covariance (:func:`teb_covsqrt`).  On power-of-two sides the shard runs as ``oa_mc_run_mv`` calls (leg-band draw, the ``oa_qe_mv``
    launch sequence, one ``oa_bin_power_multi`` pass, one moment launch; nothing leaves the device).  Elsewhere, or with
    ``one_call=False``, it runs a host loop of the existing entries with the same seeds and streams: ``Engine.grf_mix``,
    ``reconstruct_hc`` per estimator, the weighted sum, ``Engine.bin_power`` per spectrum, ``Statistics.add``.

    ``one_call``: None (default) = the one call on power-of-two sides, the host loop elsewhere.  ``one_call=True`` opts in to the one
    call on sides 2^a 3^b 5^c as well: it runs on the band grid of the estimator set (``qest.one_call_pol(estimators,
    ext_norm=True)``; ``oa_qe_band_bind`` + ``oa_mc_mv_band_bind`` bind the planes, re-bound whenever anything else used the plan in
    between -- :meth:`sample_host` included, so the two paths may be interleaved), and raises where there is no such path (chirp-z
    sides, unbounded filters, a band grid not smaller than the map): pass ``one_call=False`` there.

    ``window``: a (Ny, Nx) real-space apodisation (``maps.get_taper(shape, ...)[0]``) multiplied into the T, Q, U maps of every
    realisation before their transforms, as the reference's analysis flow does.  The window acts on Q and U, not on E and B: a taper
    leaks E into B, which the EB and TB filters do not expect, so the N0 and the mean field of EB, TB and MV on an apodised patch are
    not those of the unwindowed run.  Realisations are then drawn over the full plane, rotated E, B -> Q, U, inverse-transformed,
    windowed, transformed and rotated back Q, U -> E, B; both rotations use ``qest._qu_rot(False)`` -- the angle convention cancels
    between them, so there is no ``iau`` argument.  ``window_moments`` = (mean w^2, mean w^4); bandpowers of kappa_hat (quadratic in the
    maps) carry a factor mean(w^4) that :meth:`debiased_mean` divides out.

    ``mean_field=True``: device stacks of every estimator's kappa_hat and -- with ``mv`` -- of the MV combination in ``self.acc`` under
    the labels "mf_TT", ..., "mf_MV" (shape (ny, kp, 2), interleaved re / im, support = kappa's band, so the all-reduce moves the
    band only).

    With a window or a mean field the one call is ``oa_mc_run_mv_windowed``: ``one_call=None`` runs it on power-of-two sides and the
    host loop elsewhere, ``one_call=True`` on other sides raises.  ``one_call="band"`` behaves as ``True`` everywhere and, in addition,
    runs that call on the band grid of sides 2^a 3^b 5^c (the bindings and bands of the unwindowed one call above; per realisation the
    full-plane T, Q, U draw, one batched inverse column launch, the windowed row pass and the pruned column transform with the
    Q, U -> E, B rotation on the map's grid, the estimators on the inner grid, the stacks on the map's grid with support = the kappa
    mask's); it raises, naming ``one_call=False``, where there is no band grid.  Any other string is a ``ValueError``.  The host loop
    (any side; the reference of the one call) is then ``Engine.grf_mix(rot=(c, -s))`` on full planes, ``Engine.irfft(window=...)`` per
    field, ``Engine.rfft``, ``Engine.rot2(c, s, ...)``, the per-estimator sequence above, and the stacks added with torch."""

    def __init__(self, qest, total_power_half, bin_edges, estimators=("TT", "TE", "EE", "EB", "TB"), cross=True, mv=True, comm=None,
                 base_seed=1234, one_call=None, window=None, mean_field=False):
        torch = _torch()
        from .lensing import pol_bands
        self.q = qest
        e = self.eng = qest.eng
        self.comm = comm if comm is not None else _mpi.get_world()
        self.base_seed = int(base_seed)
        self.estimators = tuple(estimators)
        self.spectra, self.pairs = pol_spectrum_list(self.estimators, cross, mv)
        self.mv = bool(mv)
        if isinstance(one_call, str) and one_call != "band":
            raise ValueError("one_call must be None, True, False or \"band\", not %r" % (one_call,))
        self.band_call = one_call == "band"   # True, and oa_mc_run_mv_windowed on the band grid of sides 2^a 3^b 5^c as well
        self.one_call = e.pow2 if one_call is None else bool(one_call)
        self.mean_field = bool(mean_field)
        self.mf_labels = ["mf_" + XY for XY in self.estimators] + (["mf_MV"] if self.mv else [])
        self.window = None
        self.window_moments = (1.0, 1.0)
        self.rot = None
        self.host_maps = None         # host loop with a window: the windowed real T, Q, U maps of the last sample_host call
        if (window is not None or self.mean_field) and self.one_call and not e.pow2 and not self.band_call:
            from ._lib import OrphicsAmdError
            raise OrphicsAmdError("GaussianN0MonteCarloPol: with one_call=True a window or a mean-field stack runs in one call "
                                  "(oa_mc_run_mv_windowed) on power-of-two map sides only; %d x %d: construct the driver with one_call=False "
                                  "(host loop of the existing entries, any side), leave one_call=None, or opt in to the call on the band grid of "
                                  "sides 2^a 3^b 5^c with one_call=\"band\"" % (e.ny, e.nx))
        if window is not None:
            w = np.asarray(window, dtype=np.float64)
            if w.shape != (e.ny, e.nx):
                raise ValueError("window must be a (Ny, Nx) real-space array")
            self.window = e.to_real(w)
            self.window_moments = (float(np.mean(w ** 2)), float(np.mean(w ** 4)))
            c, s_ = qest._qu_rot(False)
            self.rot = (c, s_, -s_)   # Q, U -> E, B planes (oa_rot2's combination) and the negated sine of the inverse rotation
        geom = qest.geom
        nE = len(self.estimators)
        # unnormalised DFT of a unit-pixel-variance white map has |k|^2 = Npix; power p -> k = sqrt(p Npix^2/area) w
        scale = np.sqrt(float(e.npix) ** 2 / geom.area)
        a, b, c, d = (qest._hcreal(e, x * scale) for x in teb_covsqrt(total_power_half))
        self.cs = [[a, None, None], [b, c, None], [None, None, d]]
        G = [qest._setup_general(XY) for XY in self.estimators]
        self._G = G
        # pure normalisations in ONE allocation: evenly spaced planes let the divergence of all estimators run as one launch
        self.fn = e.hcreal(nE)
        for i, g_ in enumerate(G):
            self.fn[i].copy_(g_["Fnorm"])
        self.w = None
        if self.mv:
            w = qest.mv_weights(self.estimators)
            self.w = e.hcreal(nE)
            for i, XY in enumerate(self.estimators):
                self.w[i].copy_(qest._hcreal(e, w[XY]))
        self.wl, self.wk, self.rl, self.rk = pol_bands(G)
        self._bands = (self.wl, self.wk, self.rl, self.rk)
        if self.one_call and not e.pow2:
            if not qest.one_call_pol(self.estimators, ext_norm=True):
                from ._lib import OrphicsAmdError
                raise OrphicsAmdError("GaussianN0MonteCarloPol: no one-call path on this %d x %d geometry (chirp-z sides, unbounded filters or a "
                                      "band grid not smaller than the map): construct the driver with one_call=False" % (e.ny, e.nx))
            # BAND GRID: kappa's band is the kappa mask's support, which also bounds the MV weights (what one_call_pol resolved)
            self._bands = qest._pol_bands(self.estimators, True)
        self.edges = np.asarray(bin_edges, dtype=np.float64)
        self.ids = e.modl_digitize(torch.as_tensor(self.edges, device=e.device), half=True)
        self.nids = self.edges.size + 1
        self.d = self.nids - 2
        self.D = len(self.spectra) * self.d
        self.norm = geom.area / float(e.npix) ** 2
        # data-independent mode counts per bin over the whole half plane
        zero = e.hc()
        self.counts = e.bin_power(zero, zero, self.norm, self.ids, self.nids, herm=True)[1]
        self.acc = Statistics(comm=self.comm if hasattr(self.comm, "dist") else None, device=e.device)
        self._host = None
        self._c_args = None
        self._token = object()        # identity of this driver for the plan-level Monte-Carlo binding (its ids and weights planes)

    # ---- the one-call path ------------------------------------------------------------------------------------------------------
    def _entry_args(self):
        import ctypes
        if self._c_args is None:
            pcs = [pc for g_ in self._G for pc in g_["pieces"]]
            n, nE, nS = len(pcs), len(self.estimators), len(self.spectra)
            idx = {"T": 0, "E": 1, "B": 2}
            ptr = lambda t: t.data_ptr() if t is not None else None
            self._c_args = dict(
                cs=(ctypes.c_void_p * 9)(*[ptr(self.cs[i][j]) for i in range(3) for j in range(3)]),
                npieces=(ctypes.c_int * nE)(*[len(g_["pieces"]) for g_ in self._G]),
                signs=(ctypes.c_double * n)(*[float(pc[0]) for pc in pcs]),
                fgs=(ctypes.c_void_p * n)(*[pc[1].data_ptr() for pc in pcs]),
                fhs=(ctypes.c_void_p * n)(*[pc[2].data_ptr() for pc in pcs]),
                swaps=(ctypes.c_int * n)(*[1 if pc[3] else 0 for pc in pcs]),
                xsrc=(ctypes.c_int * nE)(*[idx[XY[0]] for XY in self.estimators]),
                ysrc=(ctypes.c_int * nE)(*[idx[XY[1]] for XY in self.estimators]),
                fns=(ctypes.c_void_p * nE)(*[self.fn[i].data_ptr() for i in range(nE)]),
                a=(ctypes.c_int * nS)(*[p_[0] for p_ in self.pairs]), b=(ctypes.c_int * nS)(*[p_[1] for p_ in self.pairs]))
        return self._c_args

    def _run_block(self, lo, hi, n, S, C):
        from ._lib import check
        from .engine import _ptr, _stream
        e, q, A = self.eng, self.q, self._entry_args()
        e._ordered()
        if e.pow2:
            check(e.lib.oa_plan_set_col_grid(e.plan, int(q.mcol)))       # plans are shared per geometry: policy per call
            if getattr(e, "_pipe_owner", None) is not q._token:
                e._pipe_owner = None
        wstride = self.w[0].numel() if self.w is not None else 0
        wl, wk, rl, rk = self._bands
        if e.mixed:
            # the estimator set with its pure normalisations in order, then the weights and bin ids, on the plan's inner grid; the plan
            # is shared: both are bound again whenever anything else bound it in between (sample_host's reconstruct_hc does)
            nE, nS = len(self.estimators), len(self.spectra)
            q._pol_bind(self.estimators, [self.fn[i] for i in range(nE)], self._bands, split=False)
            key = (self._token, self.w.data_ptr() if self.w is not None else 0, wstride, self.ids.data_ptr(), self.nids, nE, nS)
            own = getattr(e, "_mc_owner", None)
            if own is None or own[0] is not e._pol_owner or own[1] != key:
                e._mc_owner = None
                check(e.lib.oa_mc_mv_band_bind(e.plan, _ptr(self.w), wstride, nE, _ptr(self.ids), self.nids, nS))
                e._mc_owner = (e._pol_owner, key)
        if self.window is not None or self.mean_field:
            import ctypes
            mfs = self._stacks()
            mfp = (ctypes.c_void_p * len(mfs))(*[t.data_ptr() for t in mfs]) if mfs else None
            rot = self.rot if self.rot is not None else (None, None)
            check(e.lib.oa_mc_run_mv_windowed(e.plan, self.base_seed, int(lo), int(hi), A["cs"], len(self.estimators), A["npieces"], A["signs"],
                                              A["fgs"], A["fhs"], A["swaps"], A["xsrc"], A["ysrc"], A["fns"], _ptr(self.w), wstride,
                                              len(self.spectra), A["a"], A["b"], _ptr(self.ids), self.nids, _ptr(self.counts), float(self.norm),
                                              int(wl), int(wk), int(rl), int(rk), int(q.mrow), _ptr(self.window), _ptr(rot[0]), _ptr(rot[1]),
                                              _ptr(n), _ptr(S), _ptr(C), mfp, _stream()))
            return
        check(e.lib.oa_mc_run_mv(e.plan, self.base_seed, int(lo), int(hi), A["cs"], len(self.estimators), A["npieces"], A["signs"], A["fgs"],
                                 A["fhs"], A["swaps"], A["xsrc"], A["ysrc"], A["fns"], _ptr(self.w), wstride, len(self.spectra), A["a"], A["b"],
                                 _ptr(self.ids), self.nids, _ptr(self.counts), float(self.norm), int(wl), int(wk), int(rl), int(rk), int(q.mrow),
                                 _ptr(n), _ptr(S), _ptr(C), _stream()))

    # ---- the host loop of existing entries (every side the estimators run on; the reference of the one-call path) -------------------
    def _stacks(self):
        """the device mean-field stacks in label order (estimators, then MV); [] without ``mean_field``"""
        if not self.mean_field:
            return []
        e = self.eng
        # kappa's band of the path that writes the stacks: on a band grid the kappa mask's support (self._bands), what the kernel writes
        wk, rk = (self._bands[1], self._bands[3]) if (self.one_call and e.mixed) else (self.wk, self.rk)
        sup = (rk, wk) if (wk and rk) else None
        return [self.acc.device_stack(lab, (e.ny, e.kp, 2), support=sup) for lab in self.mf_labels]

    def _host_fields(self, i):
        """realisation ``i``'s kappa_hat planes through the existing entries: one per estimator, then -- ``mv`` -- the weighted sum"""
        torch = _torch()
        e, q = self.eng, self.q
        if self._host is None:
            t = torch.empty((3, e.ny, e.kp), dtype=e.cdt, device=e.device)
            self._host = ([t[j] for j in range(3)], [q.new_output() for _ in self.estimators], self.counts[1:-1].double())
            if self.window is not None:
                self.host_maps = [e.real() for _ in range(3)]
        draw, outs, cnt = self._host
        if self.window is None:
            e.grf_mix(self.base_seed, self.cs, out=draw, stream_id0=3 * int(i))
            f = {"T": draw[0], "E": draw[1], "B": draw[2]}
        else:
            # T, E, B -> T, Q, U in the draw's pass, x window in real space, back to T, E, B: the window multiplies Q and U
            kT, kE, kB = _windowed_teb(e, self.base_seed, self.cs, self.rot, self.window, draw, self.host_maps, 3 * int(i))
            f = {"T": kT, "E": kE, "B": kB}
        fields = [q.reconstruct_hc(XY, f[XY[0]], f[XY[1]], out=outs[j]) for j, XY in enumerate(self.estimators)]
        if self.mv:
            kmv = self.w[0] * fields[0]
            for j in range(1, len(fields)):
                kmv += self.w[j] * fields[j]
            fields = fields + [kmv]
        return fields

    def sample_host(self, i, stack=False):
        """realisation ``i``'s sample vector (device, float64) through the existing entries; ``stack`` (with ``mean_field``): its
        kappa_hat planes are added to the mean-field stacks as well"""
        torch = _torch()
        e = self.eng
        fields = self._host_fields(i)
        cnt = self._host[2]
        x = []
        for (a, b) in self.pairs:
            s, _ = e.bin_power(fields[a], fields[b], self.norm, self.ids, self.nids, herm=True, active_cols=self.wk, active_rows=self.rk)
            x.append(s[1:-1] / cnt)
        if stack:
            for t, k in zip(self._stacks(), fields):
                t += torch.view_as_real(k).to(torch.float64)
        return torch.cat(x)

    def run_local(self, sims):
        """Process the given global sim indices on this rank's GPU: every contiguous block of indices is ONE ``oa_mc_run_mv`` call,
        or -- host loop -- one :meth:`sample_host` + ``Statistics.add`` per index."""
        sims = [int(i) for i in sims]
        if not sims:
            return self
        if not self.one_call:
            for i in sims:
                self.acc.add("n0", self.sample_host(i, stack=self.mean_field))
            self._note_stacked(len(sims))
            return self
        n, S, C = self.acc.device_moments("n0", self.D)
        for lo, hi in _blocks(sims):
            self._run_block(lo, hi, n, S, C)
        self.acc.note_samples("n0", len(sims))
        self._note_stacked(len(sims))
        return self

    def _note_stacked(self, k):
        if self.mean_field:
            self._stacks()
            for lab in self.mf_labels:
                self.acc.note_stacked(lab, k)

    def run(self, nsims):
        """Shard ``nsims`` with mpi.mpi_distribute, run, reduce once; returns the reduced :class:`Statistics` (label "n0"; with
        ``mean_field`` the stacks "mf_TT", ..., "mf_MV")."""
        return _run_sharded(self, nsims)

    def _slot(self, a, b=None):
        key = (a, a if b is None else b)
        if key not in self.spectra and (key[1], key[0]) in self.spectra:
            key = (key[1], key[0])
        if key not in self.spectra:
            raise KeyError("no spectrum %s x %s in this run (spectra: %s)" % (key[0], key[1], self.spectra))
        k = self.spectra.index(key)
        return slice(k * self.d, (k + 1) * self.d)

    def mean(self, a, b=None):
        """N0^{ab} bandpowers of the (reduced) run: ``mean("EB")`` an auto, ``mean("TT", "TE")`` a cross, ``mean("MV")`` the MV auto"""
        return self.acc.mean("n0")[self._slot(a, b)]

    def debiased_mean(self, a, b=None):
        """:meth:`mean` divided by mean(w^4) of the window (1 without one)"""
        return self.mean(a, b) / self.window_moments[1]

    def sem(self, a, b=None):
        """standard error of :meth:`mean` from the run's own covariance"""
        sl = self._slot(a, b)
        return np.sqrt(np.diag(self.acc.cov("n0"))[sl] / self.acc.count("n0"))

    def cov(self):
        """D x D covariance of the sample vector (D = len(spectra) * number of bins)"""
        return self.acc.cov("n0")

    @property
    def centers(self):
        return (self.edges[1:] + self.edges[:-1]) / 2.


class LensedSimsMonteCarlo(object):
    """The reference's verification loop (tutorials/tt_verification.ipynb cells 4-5) as a sharded,
    device-resident driver: per realisation

        FlatLensingSims.get_sim (unlensed T,Q,U GRF -> lensing by an independent kappa GRF -> beam -> + noise; lensing.py:499-521)
        -> T, E, B transforms (FourierCalc.power2d is used only for these in the notebook)
        -> kappa_hat per estimator (qest.kappa_from_map(XY, ..., alreadyFTed=True, returnFt=True))
        -> C_b^{kappa_hat x kappa_in}, C_b^{kappa_in kappa_in} (FourierCalc.power2d + bin2D.bin)
        -> Statistics: sample = (C_b^x - C_b^in) / C_b^in per estimator (+ the two bandpower vectors themselves)

    with nothing but the (nbins,) vectors ever leaving the kernels' planes (device-side Statistics), realisations sharded
    by mpi_distribute and ONE reduce at the end.  ``stage_times=True`` brackets the stages with HIP events."""

    def __init__(self, sims, qest, bin_edges, estimators=("TT", "EB"), comm=None, base_seed=2024, lens_order=5, paired=False,
                 kappa_scale=1.0):
        """paired: every realisation is lensed TWICE, by +kappa and by -kappa, with the SAME unlensed CMB and the SAME noise;
        the estimator's odd part (kappa_hat[+] - kappa_hat[-]) / 2 keeps the terms of odd order in kappa -- the linear
        response plus O(kappa^3) -- while the Gaussian reconstruction noise (the N0 scatter that dominates the unpaired
        samples) and every even-order term cancel exactly: the normalisation is tested at the 1e-3 level with tens of
        simulations.  kappa_scale: amplitude factor on the input kappa; the O(kappa^3) part of the paired bias scales as
        kappa_scale^2, a normalisation error does not scale at all -- two values attribute a residual."""
        torch = _torch()
        self.paired, self.kappa_scale = bool(paired), float(kappa_scale)
        from . import maps
        self.sims, self.q, self.estimators = sims, qest, tuple(estimators)
        self.comm = comm if comm is not None else _mpi.get_world()
        self.base_seed, self.lens_order = int(base_seed), int(lens_order)
        e = self.eng = qest.eng
        geom = qest.geom
        self.pol = len(sims.shape) > 2 and sims.shape[-3] == 3
        if any(x != "TT" for x in self.estimators) and not self.pol:
            raise ValueError("polarised estimators need FlatLensingSims(pol=True)")
        self.fc = maps.FourierCalc(sims.shape, geom, iau=qest.iau, layout="half")
        self._rec_out = {}
        self.edges = np.asarray(bin_edges, dtype=np.float64)
        self.ids = e.modl_digitize(torch.as_tensor(self.edges, device=e.device), half=True)
        self.nids = self.edges.size + 1
        self.norm = geom.area / float(e.npix) ** 2
        # modes beyond the last bin edge only feed the overflow bin, which no sample uses: the binning kernels visit the leading
        # columns / the row band that hold every mode with ell <= edges[-1] (5 % of a 4096^2 0.5' plane for edges up to 3500)
        inside = np.asarray(geom.modlmap())[:, :e.nxh + 1] <= self.edges[-1]
        cols = np.nonzero(inside.any(axis=0))[0]
        rows = np.nonzero(inside.any(axis=1))[0]
        cw = int(cols.max()) + 1 if cols.size else 1
        rw = int(np.minimum(rows, e.ny - rows).max()) + 1 if rows.size else 1
        self._bin_region = dict(active_cols=0 if cw >= e.nxh + 1 else cw, active_rows=0 if 2 * rw - 1 >= e.ny else rw)
        self.acc = Statistics(comm=self.comm if hasattr(self.comm, "dist") else None, device=e.device)
        self.stage_ms = {}
        self.fast_sims = True         # FlatLensingSims.get_sim_teb (no transform taken twice); False: get_sim + iqu2teb, as the notebook writes it

    def _seed(self, kind, i):
        return (self.base_seed, kind, int(i))

    def run_local(self, sims_idx, stage_times=False):
        torch = _torch()
        e, q = self.eng, self.q
        ev = []

        def mark(name):
            if stage_times:
                t = torch.cuda.Event(enable_timing=True)
                t.record()
                ev.append((name, t))
        for i in sims_idx:
            mark("start")
            if self.paired:
                self._paired_sample(i)
                continue
            if self.fast_sims and hasattr(self.sims, "get_sim_teb") and not self.sims._fixed and not self.sims.iau_mismatch(q):
                # no transform taken twice (FlatLensingSims.get_sim_teb): the observed T, E, B transforms and kappa_in's directly
                teb, kin = self.sims.get_sim_teb(seed_cmb=self._seed(1, i), seed_kappa=self._seed(2, i), seed_noise=self._seed(3, i),
                                                 lens_order=self.lens_order)
                mark("get_sim")
                mark("transforms")
            else:
                parts = self.sims.get_sim(seed_cmb=self._seed(1, i), seed_kappa=self._seed(2, i), seed_noise=self._seed(3, i),
                                          lens_order=self.lens_order, return_intermediate=True)
                kappa, observed = parts[1], parts[5]
                mark("get_sim")
                teb = self.fc.iqu2teb(observed, normalize=False).t      # (3, Ny, kp) or (Ny, kp) hc planes: T, E, B
                if teb.ndim == 2:
                    teb = teb[None]
                kin = e.rfft(kappa.contiguous())
                mark("transforms")
            s_in, counts = e.bin_power(kin, kin, self.norm, self.ids, self.nids, herm=True, **self._bin_region)
            auto = s_in[1:-1] / counts[1:-1].double()
            self.acc.add("input", auto)
            f = {"T": teb[0], "E": teb[1] if self.pol else None, "B": teb[2] if self.pol else None}
            for XY in self.estimators:
                # one estimator-owned output plane per estimator, reused by every realisation: the pruned kernels write kappa_hat's
                # active region, the zero-fill of the rest (a 134 MB fill per call at 4096^2 float64) happens once
                if XY not in self._rec_out:
                    self._rec_out[XY] = q.new_output()
                out = self._rec_out[XY]
                if XY == "TT":
                    rec = q.reconstruct_tt_hc(f["T"], out=out)
                else:
                    rec = q.reconstruct_hc(XY, f[XY[0]], f[XY[1]], out=out)
                mark("qe_" + XY)
                s_x, _ = e.bin_power(rec, kin, self.norm, self.ids, self.nids, herm=True, **self._bin_region)
                cross = s_x[1:-1] / counts[1:-1].double()
                self.acc.add(XY, (cross - auto) / auto)
                self.acc.add("cross_" + XY, cross)
                mark("bandpowers")
        if stage_times and ev:
            torch.cuda.synchronize()
            tot = {}
            for (n0, t0), (n1, t1) in zip(ev[:-1], ev[1:]):
                if n1 == "start":
                    continue
                tot[n1] = tot.get(n1, 0.0) + t0.elapsed_time(t1)
            self.stage_ms = {k: v / max(1, len(sims_idx)) for k, v in tot.items()}
        return self

    def _paired_sample(self, i):
        e, q, sims = self.eng, self.q, self.sims
        unl = sims.get_unlensed(self._seed(1, i))
        kappa = sims.get_kappa(self._seed(2, i)) * self.kappa_scale
        ay, ax = sims.lenser.alpha_from_kappa(kappa)
        noise = sims.ngen.get_map(seed=self._seed(3, i))
        kin = e.rfft(kappa.contiguous())
        s_in, counts = e.bin_power(kin, kin, self.norm, self.ids, self.nids, herm=True)
        auto = s_in[1:-1] / counts[1:-1].double()
        self.acc.add("input", auto)
        recs = {XY: [] for XY in self.estimators}
        for sgn in (1.0, -1.0):
            alpha = (ay, ax) if sgn > 0 else (-ay, -ax)
            observed = sims.beam_maps(sims.lens_maps(unl, alpha, self.lens_order)) + noise
            teb = self.fc.iqu2teb(observed, normalize=False).t
            if teb.ndim == 2:
                teb = teb[None]
            f = {"T": teb[0], "E": teb[1] if self.pol else None, "B": teb[2] if self.pol else None}
            for XY in self.estimators:
                rec = q.reconstruct_tt_hc(f["T"]) if XY == "TT" else q.reconstruct_hc(XY, f[XY[0]], f[XY[1]])
                recs[XY].append(rec)
        for XY in self.estimators:
            odd = (recs[XY][0] - recs[XY][1]) * 0.5
            s_x, _ = e.bin_power(odd, kin, self.norm, self.ids, self.nids, herm=True)
            cross = s_x[1:-1] / counts[1:-1].double()
            self.acc.add(XY, (cross - auto) / auto)
            self.acc.add("cross_" + XY, cross)

    def run(self, nsims, stage_times=False):
        return _run_sharded(self, nsims, stage_times=stage_times)

    def table(self):
        """per estimator: (mean bias per band, its standard error, chi^2 of the pulls, weighted mean bias +- error)"""
        out = {}
        for XY in self.estimators:
            mean = self.acc.mean(XY)
            sem = np.sqrt(self.acc.var(XY) / self.acc.count(XY))
            w = 1.0 / sem ** 2
            out[XY] = {"bias": mean, "sigma": sem, "chi2": float(np.sum((mean / sem) ** 2)), "nbands": int(mean.size),
                       "weighted_mean_bias": float(np.sum(w * mean) / np.sum(w)), "weighted_mean_sigma": float(np.sum(w) ** -0.5)}
        return out

    @property
    def centers(self):
        return (self.edges[1:] + self.edges[:-1]) / 2.


class RDN0MonteCarlo(object):
    """Realisation-dependent N0 (RDN0) of the TT estimator: the Monte Carlo that debiases the kappa_hat auto-spectrum of ONE given map
    by pairing that map with simulations through the two legs of the estimator.  It follows the fluctuation of the data's own power
    and is insensitive, at first order, to a mis-modelled total power.

    Definition.  ``QE(X, Y)`` is the unsymmetrised TT reconstruction of ``qest``'s filters, ``reconstruct_tt_hc(kX=X, kY=Y)``; ``d``
    is the data map's transform.  Realisation ``i`` draws ``s`` with Philox stream ``2 i`` and ``s'`` with stream ``2 i + 1`` (key
    ``base_seed``, total power ``total_power_half``) -- the very draws ``GaussianN0MonteCarlo`` makes for its realisations ``2 i`` and
    ``2 i + 1``.  Then::

        A   = QE(d, s)  + QE(s, d)
        B   = QE(s, s') + QE(s', s)
        p(Z)_b = bandpower b of |Z|^2 (the weights, bins and mode counts of GaussianN0MonteCarlo's bandpowers)
        x_i = [ p(A) - p(B) / 2 ,  p(B) / 2 ]        # 2 d numbers: "rdn0", then "mcn0"

    and ``x_i`` is one sample of the label ``"rdn0"`` (dimension ``2 d``, ``d = len(bin_edges) - 1``): n += 1, S += x_i,
    C += x_i x_i^T.  ``|A|^2`` is exactly the four data-simulation terms of the usual six-term RDN0; ``p(B) / 2`` has the same expectation
    as its two simulation-simulation terms ``C[ss', ss'] + C[ss', s's]`` and a smaller variance.  The second half, :meth:`mcn0`, is the
    N0 of independent pairs: it carries no data and no signal trispectrum.  The debiased spectrum of the map is
    ``p(QE(d, d)) - mean(rdn0)`` (:meth:`debiased`, :meth:`data_bandpowers`).

    ``data``: a real ``(Ny, Nx)`` map (NumPy or device tensor) or its hc transform (complex device tensor of the engine's layout);
    :meth:`set_data` binds another map on the same plan.

    ``one_call``: ``None`` (default) runs the shard as ``oa_mc_run_rdn0`` calls wherever ``qest.one_call()`` holds (power-of-two sides
    and the band grid of sides 2^a 3^b 5^c: the data's three leg planes are filtered and transformed once, by ``oa_rdn0_set_data``, a
    batch of realisations shares every launch, and the combination, the binning and the moment update are one fused tail; nothing
    leaves the device) and the host loop elsewhere.  ``one_call=False`` runs the host loop of existing entries on any side, with the
    same seeds and streams: ``Engine.grf_hc`` (twice) -> :meth:`Estimator.reconstruct_tt_sym_hc` (twice) -> ``Engine.bin_power`` (twice)
    -> ``Statistics.add``.  ``one_call=True`` raises where there is no one-call path (chirp-z sides, unbounded filters, a band grid not
    smaller than the map).

    ``window``: an ``(Ny, Nx)`` real-space apodisation applied to every SIMULATION before its transform, as ``GaussianN0MonteCarlo``'s:
    ``s = R2C(window . C2R(draw) / Npix)`` from the full-plane draw of stream ``2 i``, ``s'`` the same from stream ``2 i + 1``.  ``data``
    is taken as given -- the map as analysed, i.e. ALREADY apodised by the caller; the driver never multiplies it by the window.
    ``window_moments`` = (mean w^2, mean w^4): the bandpowers of kappa_hat are quadratic in two maps and carry mean(w^4), which
    :meth:`debiased` divides out.  With a window the data's own reconstruction has a mean field; the simulations' ``A`` and ``B`` have
    none (``s``, ``s'`` and ``d`` are independent and zero-mean), so it enters only :meth:`data_bandpowers` (``mean_field=``).
    With a window ``one_call=None`` takes the one call (``oa_mc_run_rdn0_windowed``) on both classes of sides that have one --
    power-of-two sides and the band grid of sides 2^a 3^b 5^c -- because it measured faster than the host loop at every measured geometry
    of either (2.5 to 3.5 times at 2048^2 and 4096^2, 1.3 to 1.5 times at 1200^2 and 2400^2: profiles/rdn0_windowed.jsonl), and the host
    loop elsewhere (chirp-z sides, no band grid);
    ``one_call=False`` is the host loop on any side -- ``Engine.grf_hc`` (full plane) -> ``Engine.irfft`` ->
    x window -> ``Engine.rfft`` for both draws, then the sequence above; ``one_call=True`` raises where there is no one-call path.
    Without ``window`` the class behaves exactly as before it had the argument.  The polarisation / MV driver,
    :class:`RDN0MonteCarloPol`, has no ``window`` argument: it takes its window through ``set_window``."""

    def __init__(self, qest, data, total_power_half, bin_edges, comm=None, base_seed=1234, one_call=None, window=None):
        torch = _torch()
        self.q = qest
        self.eng = e = qest.eng
        self.comm = comm if comm is not None else _mpi.get_world()
        self.base_seed = int(base_seed)
        geom = qest.geom
        amp = np.sqrt(np.asarray(total_power_half, dtype=np.float64) * float(e.npix) ** 2 / geom.area)
        self.cs = qest._hcreal(e, amp)
        self.edges = np.asarray(bin_edges, dtype=np.float64)
        self.ids = e.modl_digitize(torch.as_tensor(self.edges, device=e.device), half=True)
        self.nids = self.edges.size + 1
        self.d = self.nids - 2
        self.norm = geom.area / float(e.npix) ** 2
        self.acc = Statistics(comm=self.comm if hasattr(self.comm, "dist") else None, device=e.device)
        avail = bool(qest.one_call())
        if one_call and not avail:
            from ._lib import OrphicsAmdError
            raise OrphicsAmdError("RDN0MonteCarlo: no one-call path on this %d x %d geometry (chirp-z sides, unbounded filters or a band grid "
                                  "not smaller than the map): construct the driver with one_call=False (host loop of the existing entries)"
                                  % (e.ny, e.nx))
        self.one_call = avail if one_call is None else bool(one_call)
        self._host = None
        self._hostw = None                    # (the full-plane draw and the real map of the windowed host loop)
        self.window = None
        self.window_moments = (1.0, 1.0)
        if window is not None:
            w = np.asarray(window, dtype=np.float64)
            if w.shape != (e.ny, e.nx):
                raise ValueError("window must be a (Ny, Nx) real-space array")
            self.window = e.to_real(w)
            self.window_moments = (float(np.mean(w ** 2)), float(np.mean(w ** 4)))
        self.set_data(data)

    def set_data(self, data):
        """Bind another data map (real ``(Ny, Nx)`` map or hc transform) on the same plan, bins and simulations; the accumulated
        samples are NOT reset (use a new driver, or a fresh ``self.acc``, for an independent run)."""
        torch = _torch()
        e = self.eng
        if isinstance(data, torch.Tensor) and data.is_complex():
            kd = e._chk(data.to(e.cdt).contiguous(), "hc")
        else:
            a = data if isinstance(data, torch.Tensor) else np.asarray(data)
            if tuple(a.shape) != (e.ny, e.nx):
                raise ValueError("data must be a real (Ny, Nx) map or an hc transform of the engine's layout")
            kd = e.rfft(e.to_real(a))
        self.kd = kd
        self._dtoken = object()           # the plan's cached data legs (oa_rdn0_set_data) belong to this token
        return self

    # ---- results (after run / allreduce) ------------------------------------------------------------------------------------------
    def rdn0(self):
        """mean of the first half of the sample vector: the realisation-dependent N0 bandpowers."""
        return self.acc.mean("rdn0")[:self.d]

    def mcn0(self):
        """mean of the second half: the N0 of independent simulation pairs (no data)."""
        return self.acc.mean("rdn0")[self.d:]

    def sem(self):
        """standard error of :meth:`rdn0`."""
        return np.sqrt(self.acc.var("rdn0")[:self.d] / self.acc.count("rdn0"))

    def cov(self):
        """sample covariance of the whole ``2 d`` vector (rdn0 block, mcn0 block and their cross block)."""
        return self.acc.cov("rdn0")

    def data_bandpowers(self, mean_field=None):
        """``p(QE(d, d) - mean_field)``: the bandpowers of the data's own reconstruction, with the driver's bins.  ``mean_field``: a
        complex hc tensor of kappa_hat's layout, or the ``(Ny, kp, 2)`` interleaved (re, im) stack mean that
        ``GaussianN0MonteCarlo(window=..., mean_field=True)`` accumulates (``acc.stack_mean("mf")``); None subtracts nothing."""
        torch = _torch()
        q, e = self.q, self.eng
        kap = q.reconstruct_tt_hc(self.kd)
        if mean_field is not None:
            m = mean_field if isinstance(mean_field, torch.Tensor) else torch.as_tensor(np.asarray(mean_field))
            m = m.to(e.device)
            if not m.is_complex():
                if tuple(m.shape) != (e.ny, e.kp, 2):
                    raise ValueError("mean_field must be a complex (Ny, kp) hc tensor or a real (Ny, kp, 2) stack mean")
                m = torch.view_as_complex(m.to(torch.float64).contiguous())
            if tuple(m.shape) != (e.ny, e.kp):
                raise ValueError("mean_field must be a complex (Ny, kp) hc tensor or a real (Ny, kp, 2) stack mean")
            kap = kap - m.to(e.cdt)
        s, _ = e.bin_power(kap, kap, self.norm, self.ids, self.nids, herm=True, active_cols=q.kappa_cols, active_rows=q.kappa_rows)
        return (s[1:-1] / self._counts()).cpu().numpy()

    def debiased(self, data_bandpowers=None, mean_field=None):
        """``(data_bandpowers - rdn0()) / window_moments[1]`` (``data_bandpowers=None``: :meth:`data_bandpowers` with ``mean_field``); the
        divisor mean(w^4) is 1 without a window."""
        p = self.data_bandpowers(mean_field) if data_bandpowers is None else np.asarray(data_bandpowers, dtype=np.float64)
        return (p - self.rdn0()) / self.window_moments[1]

    @property
    def centers(self):
        return (self.edges[1:] + self.edges[:-1]) / 2.

    # ---- the shard ----------------------------------------------------------------------------------------------------------------
    def _counts(self):
        """data-independent mode counts of the interior bins over the whole half plane (float64 device tensor)."""
        if getattr(self, "_cnt", None) is None:
            e = self.eng
            zero = e.hc()
            self._cnt = e.bin_power(zero, zero, self.norm, self.ids, self.nids, herm=True)[1][1:-1].double()
        return self._cnt

    def sample_host(self, i):
        """x_i through the existing entries (the host loop's arithmetic): float64 device tensor of ``2 d`` numbers."""
        torch = _torch()
        q, e = self.q, self.eng
        if self._host is None:
            self._host = (e.hc(), e.hc(), q.new_output(), q.new_output())
        s0, s1, ka, kb = self._host
        wl, rl = (q.leg_cols, q.leg_rows) if (q.leg_cols and q.leg_rows) else (0, 0)
        if self.window is not None:            # the full-plane draws of oa_mc_run_windowed, windowed in real space
            if self._hostw is None:
                self._hostw = (e.hc(), e.real())
            draw, tmap = self._hostw
            for z, dst in ((0, s0), (1, s1)):
                e.grf_hc(self.base_seed, 2 * i + z, self.cs, out=draw)
                e.irfft(draw, out=tmap)
                tmap.mul_(self.window)
                e.rfft(tmap, out=dst)
        else:
            e.grf_hc(self.base_seed, 2 * i, self.cs, out=s0, width=wl, rband=rl)
            e.grf_hc(self.base_seed, 2 * i + 1, self.cs, out=s1, width=wl, rband=rl)
        ka = q.reconstruct_tt_sym_hc(self.kd, s0, out=ka)
        kb = q.reconstruct_tt_sym_hc(s0, s1, out=kb)
        region = dict(active_cols=q.kappa_cols, active_rows=q.kappa_rows)
        pa = e.bin_power(ka, ka, self.norm, self.ids, self.nids, herm=True, **region)[0][1:-1] / self._counts()
        half = 0.5 * (e.bin_power(kb, kb, self.norm, self.ids, self.nids, herm=True, **region)[0][1:-1] / self._counts())
        return torch.cat((pa - half, half))

    def run_local(self, sims):
        """Process the given global realisation indices on this rank's GPU: every contiguous block of indices is ONE ``oa_mc_run_rdn0``
        call (``oa_mc_run_rdn0_windowed`` with a window; one-call path), or one :meth:`sample_host` + ``Statistics.add`` per index (host loop)."""
        from ._lib import check
        from .engine import _ptr, _stream
        sims = [int(i) for i in sims]
        if not sims:
            return self
        if not self.one_call:
            for i in sims:
                self.acc.add("rdn0", self.sample_host(i))
            return self
        q = self.q
        q.bind_bins(self.ids, self.nids, self.norm)
        e = q._bind_bins()
        if getattr(e, "_rdn0_owner", None) is not self._dtoken:
            check(e.lib.oa_rdn0_set_data(e.plan, _ptr(self.kd), _stream()))
            e._rdn0_owner = self._dtoken
        n, S, C = self.acc.device_moments("rdn0", 2 * self.d)
        for lo, hi in _blocks(sims):
            if self.window is not None:
                check(e.lib.oa_mc_run_rdn0_windowed(e.plan, self.base_seed, lo, hi, _ptr(self.cs), _ptr(self.window), _ptr(n), _ptr(S), _ptr(C),
                                                    _stream()))
            else:
                check(e.lib.oa_mc_run_rdn0(e.plan, self.base_seed, lo, hi, _ptr(self.cs), _ptr(n), _ptr(S), _ptr(C), _stream()))
        self.acc.note_samples("rdn0", len(sims))
        return self

    def run(self, nsims):
        """Shard ``nsims`` realisations with mpi.mpi_distribute, run, reduce once; returns the reduced :class:`Statistics` (one label,
        ``"rdn0"``, of dimension ``2 d``)."""
        return _run_sharded(self, nsims)


class RDN0MonteCarloPol(object):
    """Realisation-dependent N0 (RDN0) of an estimator set (TT, TE, EE, EB, TB), its cross-spectra and its minimum-variance (MV)
    combination: the bias a real analysis subtracts from the kappa_hat spectra of ONE observed T, E, B (or T, Q, U) triple.

    Definition.  For field triples ``X = (X_T, X_E, X_B)`` and ``Y``, ``QE_e(X; Y)`` is estimator ``e`` of the set with
    ``kX = X[XY[0]]`` and ``kY = Y[XY[1]]`` -- ``Estimator.reconstruct_hc(XY, X[XY[0]], Y[XY[1]])``.  ``d`` is the data triple.
    Realisation ``i`` draws ``s`` = ``Engine.grf_mix(stream_id0 = 6 i)`` (Philox streams ``6 i .. 6 i + 2`` for T, E, B) and ``s'`` =
    ``Engine.grf_mix(stream_id0 = 6 i + 3)`` (streams ``6 i + 3 .. 6 i + 5``), key ``base_seed``, total powers ``total_power_half``:
    the draws :class:`GaussianN0MonteCarloPol` makes for its realisations ``2 i`` and ``2 i + 1``.  Then, for every estimator ``e``::

        A_e  = QE_e(d; s)  + QE_e(s; d)            B_e  = QE_e(s; s') + QE_e(s'; s)
        A_MV = sum_e w_e A_e                       B_MV = sum_e w_e B_e                 (w = qest.mv_weights(estimators))
        p(Z_a, Z_b)_j = bandpower j of Re(Z_a conj Z_b)      (weights, bins, mode counts of GaussianN0MonteCarloPol's bandpowers)
        x_i = [ p(A_a, A_b) - p(B_a, B_b) / 2  for every spectrum (a, b) of ``spectra`` ]       # "rdn0": nspec * d numbers
           ++ [ p(B_a, B_b) / 2                for every spectrum (a, b) of ``spectra`` ]       # "mcn0": nspec * d numbers

    and ``x_i`` is one sample of the label ``"rdn0"`` (dimension ``2 * nspec * d``, ``d = len(bin_edges) - 1``): n += 1, S += x_i,
    C += x_i x_i^T.  ``spectra`` is :func:`pol_spectrum_list` ``(estimators, cross, mv)``.  ``p(A_a, A_b)`` is the sum of the four
    data-simulation terms of the six-term RDN0 of the cross-spectrum (a, b); the mcn0 half carries no data.  The debiased spectrum of
    the data is ``p(QE_a(d; d), QE_b(d; d)) - mean(rdn0_ab)`` (:meth:`debiased`, :meth:`data_bandpowers`).  For
    ``estimators=("TT",)`` this is :class:`RDN0MonteCarlo`'s definition with other Philox streams.

    ``data``: three hc transforms (T, E, B) of the engine's layout, or -- ``qu=True`` -- three real ``(Ny, Nx)`` maps T, Q, U, converted
    once with ``Engine.rfft`` and the per-mode rotation ``reconstruct_mv_from_maps(qu=True)`` uses (``iau``: the angle convention).
    :meth:`set_data` binds another triple on the same plan.

    ``one_call``: ``True`` runs the shard as ``oa_mc_run_rdn0_mv`` calls on power-of-two sides (the data's distinct leg planes are
    transformed once by ``oa_rdn0_set_data_mv``; per realisation two band draws, the leg planes of s and s', the row stage of the
    2 nest chains, their divergences and one combine / bin / moments tail; nothing leaves the device) and raises elsewhere: band-grid
    sides (2^a 3^b 5^c) run the host loop for now, as do chirp-z sides.  ``one_call=False`` runs the host loop of existing entries on
    any side with the same seeds and streams: ``Engine.grf_mix`` (twice), per estimator four ``reconstruct_hc`` calls (the second of
    each pair with ``accumulate=True``), the weighted sums in torch, ``Engine.bin_power`` per spectrum for A and for B,
    ``Statistics.add``.  ``one_call=None`` (default): the one call on power-of-two sides, the host loop elsewhere.
    ``one_call="band"`` (:class:`GaussianN0MonteCarloPol`'s spelling and meaning) is the opt-in to the one call on sides 2^a 3^b 5^c: on
    power-of-two sides it behaves as ``True``; elsewhere the shard runs on the band grid of the estimator set
    (``qest.one_call_pol(estimators, ext_norm=True)``, bands ``qest._pol_bands(estimators, True)``: kappa's band is the kappa mask's
    support) -- per block ``oa_qe_band_bind``, ``oa_mc_mv_band_bind`` and ``oa_rdn0_set_data_mv`` where the plan's bindings are not this
    driver's current ones (a :meth:`sample_host` or :meth:`data_bandpowers` call in between re-binds the plan per estimator; the driver
    then binds and sets the data again by itself), then ``oa_mc_run_rdn0_mv``: per realisation ONE draw launch for both triples
    (``oa_grf_mix_band_inner_triples``) and the launches above on the inner grid.  It raises ``OrphicsAmdError`` naming
    ``one_call=False`` where there is no band grid (chirp-z sides, unbounded filters, a grid not smaller than the map); any other string
    is a ``ValueError``.  The windowed one call is not on the band grid: :meth:`set_window` raises there on a ``"band"`` driver.

    There is no window argument to the constructor: bind one with :meth:`set_window` (before any sample is accumulated).  ``s`` and
    ``s'`` are then the WINDOWED triples :class:`GaussianN0MonteCarloPol` ``(window=...)`` makes for its realisations ``2 i`` and
    ``2 i + 1``: the full-plane draw rotated E, B -> Q, U, inverse-transformed, multiplied by the window, transformed and rotated back
    (the window multiplies T, Q, U, not E, B: a taper leaks E into B).  ``data`` is taken as given -- the triple as analysed, i.e.
    ALREADY apodised by the caller.  ``window_moments`` = (mean w^2, mean w^4); :meth:`debiased` divides mean(w^4) out.  With a window
    ``one_call=True`` runs ``oa_mc_run_rdn0_mv_windowed`` on power-of-two sides (the source stage of ``oa_mc_run_mv_windowed`` per triple,
    or -- plan option ``draw_fused`` = 1 -- per realisation ONE inverse column pass-1 launch that evaluates both triples' draws at its
    load, each Philox counter once per triple: ``oa_grf_mix_icols``, then one pass 2, one fused row launch C2R x window -> R2C and one
    forward column launch over the six planes, the Q, U -> E, B rotation on the leg band; then the launches above).  ``one_call=None``
    with a window is the host loop on every side until the one call has been timed against it (``ONE_CALL_WINDOWED_DEFAULT``).  The host loop and :meth:`sample_host` (the reference of the one call) are
    then, per draw ``z``: ``Engine.grf_mix(rot=(c, -s), stream_id0=6 i + 3 z)`` on full planes, ``Engine.irfft(window=...)`` per field,
    ``Engine.rfft``, ``Engine.rot2``, then the sequence above.  The data's own reconstructions carry the window's mean field; the
    simulations' ``A`` and ``B`` carry none (``s``, ``s'``, ``d`` are independent and zero-mean): :meth:`data_bandpowers` takes the stacks
    ``GaussianN0MonteCarloPol(window=..., mean_field=True)`` accumulates.  Without :meth:`set_window` every method behaves exactly as
    before the method existed."""

    def __init__(self, qest, data, total_power_half, bin_edges, estimators=("TT", "TE", "EE", "EB", "TB"), cross=True, mv=True, comm=None,
                 base_seed=1234, one_call=None, qu=False, iau=False):
        if isinstance(one_call, str) and one_call != "band":
            raise ValueError("one_call must be None, True, False or \"band\", not %r" % (one_call,))
        self.band_call = one_call == "band"   # True, and oa_mc_run_rdn0_mv on the band grid of sides 2^a 3^b 5^c as well
        # covsqrt, pure normalisations in one allocation, weights, bands, ids, counts: GaussianN0MonteCarloPol's set-up, host-loop flavour
        g = self._set = GaussianN0MonteCarloPol(qest, total_power_half, bin_edges, estimators=estimators, cross=cross, mv=mv, comm=comm,
                                                base_seed=base_seed, one_call=False)
        self.q, self.eng, self.comm, self.base_seed = qest, g.eng, g.comm, g.base_seed
        e = self.eng
        self.estimators, self.spectra, self.pairs, self.mv = g.estimators, g.spectra, g.pairs, g.mv
        self.edges, self.ids, self.nids, self.d, self.norm = g.edges, g.ids, g.nids, g.d, g.norm
        self.cs, self.w, self.counts = g.cs, g.w, g.counts
        self.nspec = len(self.spectra)
        self.D = 2 * self.nspec * self.d
        if one_call and not e.pow2 and not self.band_call:
            from ._lib import OrphicsAmdError
            raise OrphicsAmdError("RDN0MonteCarloPol: with one_call=True the one call (oa_mc_run_rdn0_mv) runs on power-of-two map sides only; "
                                  "%d x %d: construct the driver with one_call=False (host loop of the existing entries, any side), leave "
                                  "one_call=None, or opt in to the call on the band grid of sides 2^a 3^b 5^c with one_call=\"band\""
                                  % (e.ny, e.nx))
        self._bands = g._bands
        if self.band_call and not e.pow2:
            if not qest.one_call_pol(self.estimators, ext_norm=True):
                from ._lib import OrphicsAmdError
                raise OrphicsAmdError("RDN0MonteCarloPol: no one-call path on this %d x %d geometry (chirp-z sides, unbounded filters or a "
                                      "band grid not smaller than the map): construct the driver with one_call=False" % (e.ny, e.nx))
            # BAND GRID: kappa's band is the kappa mask's support, which also bounds the MV weights (what one_call_pol resolved)
            self._bands = qest._pol_bands(self.estimators, True)
        self.one_call = bool(e.pow2) if one_call is None else bool(one_call)
        self.qu, self.iau = bool(qu), bool(iau)
        self.acc = Statistics(comm=self.comm if hasattr(self.comm, "dist") else None, device=e.device)
        self._host = None
        self._hostw = None                    # (the real T, Q, U maps of the windowed host loop)
        self._one_call_asked = True if self.band_call else one_call
        self._nsamples = 0
        self.window = None
        self.window_moments = (1.0, 1.0)
        self.rot = None
        self.set_data(data)

    def set_window(self, window):
        """Bind the data's apodisation window, an ``(Ny, Nx)`` real array (``None`` removes it): every SIMULATION is multiplied by it in
        real space (T, Q, U) before its transform; the data is never touched.  Sets ``window``, ``window_moments`` = (mean w^2,
        mean w^4) and the Q, U -> E, B rotation planes ``qest._qu_rot(False)``.  Windowed and unwindowed samples must not share a label:
        raises once samples have been accumulated.  Returns ``self``."""
        e = self.eng
        if self._nsamples:
            raise RuntimeError("RDN0MonteCarloPol.set_window: %d samples are already accumulated; windowed and unwindowed samples must not "
                               "share a label -- bind the window before run / run_local, or build another driver" % self._nsamples)
        if window is None:
            self.window, self.window_moments, self.rot = None, (1.0, 1.0), None
        else:
            if self.band_call and not e.pow2:
                from ._lib import OrphicsAmdError
                raise OrphicsAmdError("RDN0MonteCarloPol.set_window: the windowed one call (oa_mc_run_rdn0_mv_windowed) runs on power-of-two map "
                                      "sides only, not on the band grid of a one_call=\"band\" driver; %d x %d: construct the driver with "
                                      "one_call=False (host loop of the existing entries, any side)" % (e.ny, e.nx))
            w = np.asarray(window, dtype=np.float64)
            if w.shape != (e.ny, e.nx):
                raise ValueError("window must be a (Ny, Nx) real-space array")
            self.window = e.to_real(w)
            self.window_moments = (float(np.mean(w ** 2)), float(np.mean(w ** 4)))
            c, s_ = self.q._qu_rot(False)
            self.rot = (c, s_, -s_)       # Q, U -> E, B planes (oa_rot2's combination) and the negated sine of the inverse rotation
        self.one_call = self._default_one_call()
        return self

    def _default_one_call(self):
        # one_call=None with a window on power-of-two sides: the one call only once it has measured faster than the host loop beyond both
        # spreads at every measured geometry (tools/rdn0_pol_bench.py --windowed); no such measurement is recorded yet, so the
        # host loop stays the default there and one_call=True opts in -- ONE_CALL_WINDOWED_DEFAULT
        if self._one_call_asked is None:
            return bool(self.eng.pow2) and (self.window is None or self.ONE_CALL_WINDOWED_DEFAULT)
        return bool(self._one_call_asked)

    ONE_CALL_WINDOWED_DEFAULT = False

    def set_data(self, data):
        """Bind another data triple (hc transforms T, E, B, or real maps T, Q, U with ``qu=True``) on the same plan, bins and
        simulations; the accumulated samples are NOT reset."""
        e = self.eng
        data = list(data)
        if len(data) != 3:
            raise ValueError("data must be three planes: hc transforms (T, E, B), or real maps (T, Q, U) with qu=True")
        if self.qu:
            self.kd = list(self.q._maps_to_hc([tuple(e.to_real(m) for m in data)], True, self.iau)[0])
        else:
            self.kd = [e._chk(k.to(e.cdt).contiguous(), "hc") for k in data]
        self._dtoken = object()           # the plan's cached data legs (oa_rdn0_set_data_mv) belong to this token
        self._pd = None
        self._pd_key = None
        return self

    # ---- results (after run / allreduce) ------------------------------------------------------------------------------------------
    def _slot(self, a, b=None, half=0):
        sl = self._set._slot(a, b)
        off = half * self.nspec * self.d
        return slice(sl.start + off, sl.stop + off)

    def rdn0(self, a, b=None):
        """mean of the rdn0 block of spectrum (a, b): ``rdn0("EB")`` an auto, ``rdn0("TT", "TE")`` a cross, ``rdn0("MV")`` the MV auto."""
        return self.acc.mean("rdn0")[self._slot(a, b)]

    def mcn0(self, a, b=None):
        """mean of the mcn0 block of spectrum (a, b): the N0 of independent simulation pairs (no data)."""
        return self.acc.mean("rdn0")[self._slot(a, b, 1)]

    def sem(self, a, b=None):
        """standard error of :meth:`rdn0` from the run's own covariance."""
        return np.sqrt(np.diag(self.acc.cov("rdn0"))[self._slot(a, b)] / self.acc.count("rdn0"))

    def cov(self):
        """D x D covariance of the sample vector (D = 2 * nspec * d: the rdn0 blocks, then the mcn0 blocks)."""
        return self.acc.cov("rdn0")

    def _mean_field_planes(self, mean_field):
        """label -> complex (Ny, kp) hc tensor of the engine's dtype, from complex tensors or (Ny, kp, 2) stack means"""
        torch = _torch()
        e = self.eng
        labels = list(self.estimators) + (["MV"] if self.mv else [])
        out = {}
        for lab, m in mean_field.items():
            if lab not in labels:
                raise ValueError("mean_field: %r is not a field of this driver (%s)" % (lab, ", ".join(labels)))
            m = m if isinstance(m, torch.Tensor) else torch.as_tensor(np.asarray(m))
            m = m.to(e.device)
            if not m.is_complex():
                if tuple(m.shape) != (e.ny, e.kp, 2):
                    raise ValueError("mean_field[%r] must be a complex (Ny, kp) hc tensor or a real (Ny, kp, 2) stack mean" % lab)
                m = torch.view_as_complex(m.to(torch.float64).contiguous())
            if tuple(m.shape) != (e.ny, e.kp):
                raise ValueError("mean_field[%r] must be a complex (Ny, kp) hc tensor or a real (Ny, kp, 2) stack mean" % lab)
            out[lab] = m.to(e.cdt)
        return out

    def data_bandpowers(self, a, b=None, mean_field=None):
        """``p(QE_a(d; d) - m_a, QE_b(d; d) - m_b)``: the bandpowers of the data's own reconstructions, with the driver's bins.
        ``mean_field``: a mapping from field label (``"TT"``, ..., ``"MV"``) to a complex hc tensor of kappa_hat's layout or the
        ``(Ny, kp, 2)`` stack mean ``GaussianN0MonteCarloPol(window=..., mean_field=True)`` accumulates (``acc.stack_mean("mf_EB")``, ...);
        a label that is absent subtracts nothing, except that the MV field without a ``"MV"`` entry is the weighted sum of the
        estimators' fields AFTER their subtraction.  None subtracts nothing."""
        key = None if mean_field is None else tuple(sorted((lab, id(m)) for lab, m in mean_field.items()))
        if self._pd is None or self._pd_key != key:
            torch = _torch()
            e, q, g = self.eng, self.q, self._set
            f = dict(zip("TEB", self.kd))
            mf = self._mean_field_planes(mean_field) if mean_field is not None else {}
            fields = [q.reconstruct_hc(XY, f[XY[0]], f[XY[1]]) for XY in self.estimators]
            raw = list(fields)
            for j, XY in enumerate(self.estimators):
                if XY in mf:
                    fields[j] = fields[j] - mf[XY]
            if self.mv:
                src = raw if "MV" in mf else fields
                kmv = g.w[0] * src[0]
                for j in range(1, len(self.estimators)):
                    kmv += g.w[j] * src[j]
                if "MV" in mf:
                    kmv -= mf["MV"]
                fields.append(kmv)
            cnt = g.counts[1:-1].double()
            self._pd = torch.cat([e.bin_power(fields[i], fields[j], self.norm, self.ids, self.nids, herm=True, active_cols=g.wk,
                                              active_rows=g.rk)[0][1:-1] / cnt for (i, j) in self.pairs]).cpu().numpy()
            self._pd_key = key
            self._pd_hold = None if mean_field is None else list(mean_field.values())     # (the key holds ids: keep the objects alive)
        return self._pd[self._set._slot(a, b)]

    def debiased(self, a, b=None, mean_field=None):
        """``(data_bandpowers(a, b, mean_field) - rdn0(a, b)) / window_moments[1]``; the divisor mean(w^4) is 1 without a window."""
        return (self.data_bandpowers(a, b, mean_field) - self.rdn0(a, b)) / self.window_moments[1]

    @property
    def centers(self):
        return (self.edges[1:] + self.edges[:-1]) / 2.

    # ---- the shard ----------------------------------------------------------------------------------------------------------------
    def sample_host(self, i):
        """x_i through the existing entries (the host loop's arithmetic): float64 device tensor of ``2 * nspec * d`` numbers."""
        torch = _torch()
        e, q, g = self.eng, self.q, self._set
        nE = len(self.estimators)
        if self._host is None:
            t = torch.empty((6, e.ny, e.kp), dtype=e.cdt, device=e.device)
            self._host = ([t[j] for j in range(3)], [t[3 + j] for j in range(3)], [q.new_output() for _ in range(2 * nE)],
                          g.counts[1:-1].double())
        s0, s1, outs, cnt = self._host
        if self.window is None:
            e.grf_mix(self.base_seed, g.cs, out=s0, stream_id0=6 * int(i))
            e.grf_mix(self.base_seed, g.cs, out=s1, stream_id0=6 * int(i) + 3)
        else:                                 # the windowed triples of GaussianN0MonteCarloPol(window=...)'s realisations 2 i, 2 i + 1
            if self._hostw is None:
                self._hostw = [e.real() for _ in range(3)]
            s0 = list(_windowed_teb(e, self.base_seed, g.cs, self.rot, self.window, s0, self._hostw, 6 * int(i)))
            s1 = list(_windowed_teb(e, self.base_seed, g.cs, self.rot, self.window, s1, self._hostw, 6 * int(i) + 3))
            self.host_fields = (s0, s1)       # (the windowed T, E, B of the last sample_host call)
        idx = {"T": 0, "E": 1, "B": 2}
        sets = []
        for k, (X, Y) in enumerate(((self.kd, s0), (s0, s1))):        # A = (d, s) + (s, d); B = (s, s') + (s', s)
            fields = []
            for j, XY in enumerate(self.estimators):
                x, y = idx[XY[0]], idx[XY[1]]
                out = q.reconstruct_hc(XY, X[x], Y[y], out=outs[k * nE + j])
                fields.append(q.reconstruct_hc(XY, Y[x], X[y], out=out, accumulate=True))
            if self.mv:
                kmv = g.w[0] * fields[0]
                for j in range(1, nE):
                    kmv += g.w[j] * fields[j]
                fields.append(kmv)
            sets.append(fields)
        region = dict(active_cols=g.wk, active_rows=g.rk)
        p = [[e.bin_power(f[a], f[b], self.norm, self.ids, self.nids, herm=True, **region)[0][1:-1] / cnt for (a, b) in self.pairs] for f in sets]
        half = [0.5 * pb for pb in p[1]]
        return torch.cat([pa - h for pa, h in zip(p[0], half)] + half)

    def _run_block(self, lo, hi, n, S, C):
        import ctypes
        from ._lib import check
        from .engine import _ptr, _stream
        e, q, g = self.eng, self.q, self._set
        A = g._entry_args()
        e._ordered()
        nE = len(self.estimators)
        wl, wk, rl, rk = self._bands
        wstride = g.w[0].numel() if g.w is not None else 0
        own = (self._dtoken, int(q.mcol), int(q.mrow))
        if e.pow2:
            check(e.lib.oa_plan_set_col_grid(e.plan, int(q.mcol)))       # plans are shared per geometry: policy per call
            if getattr(e, "_pipe_owner", None) is not q._token:
                e._pipe_owner = None
        else:
            # BAND GRID: the estimator set with its pure normalisations in order, then the weights and bin ids, on the plan's inner grid
            # (GaussianN0MonteCarloPol._run_block's bindings); the data legs belong to the oa_qe_band_bind binding they were made on, so
            # their owner carries the identity of the plan's current one: whatever bound the plan in between (sample_host's and
            # data_bandpowers' reconstruct_hc do) makes this block bind and set the data again
            q._pol_bind(self.estimators, [g.fn[i] for i in range(nE)], self._bands, split=False)
            key = (g._token, g.w.data_ptr() if g.w is not None else 0, wstride, self.ids.data_ptr(), self.nids, nE, self.nspec)
            mc = getattr(e, "_mc_owner", None)
            if mc is None or mc[0] is not e._pol_owner or mc[1] != key:
                e._mc_owner = None
                check(e.lib.oa_mc_mv_band_bind(e.plan, _ptr(g.w), wstride, nE, _ptr(self.ids), self.nids, self.nspec))
                e._mc_owner = (e._pol_owner, key)
        cur = getattr(e, "_rdn0mv_owner", None)
        if e.pow2:
            fresh = cur == own
        else:                                 # (identity, not equality: a re-made binding has an equal key)
            fresh = isinstance(cur, tuple) and len(cur) == 2 and cur[0] is e._pol_owner and cur[1] == own
            own = (e._pol_owner, own)
        if not fresh:
            e._rdn0mv_owner = None
            kd = (ctypes.c_void_p * 3)(*[k.data_ptr() for k in self.kd])
            check(e.lib.oa_rdn0_set_data_mv(e.plan, kd, nE, A["npieces"], A["fgs"], A["fhs"], A["swaps"], A["xsrc"], A["ysrc"], int(wl), int(wk),
                                            int(rl), int(rk), int(q.mrow), _stream()))
            e._rdn0mv_owner = own
        if self.window is not None:
            check(e.lib.oa_mc_run_rdn0_mv_windowed(e.plan, self.base_seed, int(lo), int(hi), A["cs"], nE, A["npieces"], A["signs"], A["fgs"],
                                                   A["fhs"], A["swaps"], A["xsrc"], A["ysrc"], A["fns"], _ptr(g.w), wstride, self.nspec, A["a"],
                                                   A["b"], _ptr(self.ids), self.nids, _ptr(g.counts), float(self.norm), int(wl), int(wk), int(rl),
                                                   int(rk), int(q.mrow), _ptr(self.window), _ptr(self.rot[0]), _ptr(self.rot[1]), _ptr(n), _ptr(S),
                                                   _ptr(C), _stream()))
            return
        check(e.lib.oa_mc_run_rdn0_mv(e.plan, self.base_seed, int(lo), int(hi), A["cs"], nE, A["npieces"], A["signs"], A["fgs"], A["fhs"], A["swaps"],
                                      A["xsrc"], A["ysrc"], A["fns"], _ptr(g.w), wstride, self.nspec, A["a"], A["b"], _ptr(self.ids), self.nids,
                                      _ptr(g.counts), float(self.norm), int(wl), int(wk), int(rl), int(rk), int(q.mrow), _ptr(n), _ptr(S), _ptr(C),
                                      _stream()))

    def run_local(self, sims):
        """Process the given global realisation indices on this rank's GPU: every contiguous block of indices is ONE
        ``oa_mc_run_rdn0_mv`` call (``oa_mc_run_rdn0_mv_windowed`` with a window; one-call path), or one :meth:`sample_host` +
        ``Statistics.add`` per index (host loop)."""
        sims = [int(i) for i in sims]
        if not sims:
            return self
        self._nsamples += len(sims)
        if not self.one_call:
            for i in sims:
                self.acc.add("rdn0", self.sample_host(i))
            return self
        n, S, C = self.acc.device_moments("rdn0", self.D)
        for lo, hi in _blocks(sims):
            self._run_block(lo, hi, n, S, C)
        self.acc.note_samples("rdn0", len(sims))
        return self

    def run(self, nsims):
        """Shard ``nsims`` realisations with mpi.mpi_distribute, run, reduce once; returns the reduced :class:`Statistics` (one label,
        ``"rdn0"``, of dimension ``2 * nspec * d``)."""
        return _run_sharded(self, nsims)
