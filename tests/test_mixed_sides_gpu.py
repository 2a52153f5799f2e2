"""GPU: the mixed-radix transforms (csrc/fft_mixed.hpp, csrc/mixed.hip) across the sides oa_plan_create accepts -- every even
2^a 3^b 5^c side up to 8192 -- chosen so that each kernel branch is hit at its edge: the radix mixes, the column-tile widths
mr_col_logc picks in each precision, and the LDS limits where the two-buffer Stockham form gives way to the in-place one.
Engine.rfft / irfft / cfft / cfft(inverse=True) against numpy.fft in float64 on the same inputs, with the bounds of
test_engine_gpu.test_non_power_of_two_sides: max |got - ref| / max |ref| <= 1e-11 (float64 plans), 2e-5 (float32 plans)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-11, "f32": 2e-5}

SHAPES = [
    # smallest sides; nx/2 = 25 is odd (50), the packed row transform of 18 / 20 / 24 points
    (36, 40), (40, 48), (48, 50), (50, 36),
    # 3-heavy and 5-heavy: 1458 = 2 3^6, 4374 = 2 3^7, 1250 = 2 5^4; nx/2 odd (729, 125, 243, 375)
    (1458, 250), (250, 1458), (4374, 50), (1250, 486), (40, 750),
    # one power-of-two side next to a mixed one, both orientations; (750, 600) next to test_engine_gpu's (600, 750)
    (1024, 1200), (1200, 512), (750, 600),
    # column-tile widths C (f64 / f32) over nx/2 + 1 = 21, 25, 19 columns, never a multiple of C:
    # 96: 16 / 16, 384: 8 / 16, 750: 4 / 8, 1200: 2 / 4, 2400: 1 / 2, 3072: 1 / 2 (f32's last two-column tile: 6144 values x 8 B x 2)
    (96, 40), (384, 48), (750, 36), (1200, 40), (2400, 36), (3072, 40),
    # LDS edges of the columns: 5120 is exactly 160 KB for two f64 buffers (the last two-buffer side), 5184 the first in-place one
    (5120, 36), (5184, 36),
    # complex rows: nx = 5120 is one element over (2 (nx + 1) 16 B) for f64 cfft -> in place; 5184 next to it
    (36, 5120), (32, 5184),
    # 6250 = 2 5^5 in place (five radix-5 stages); the largest sides, thin so that the NumPy reference stays cheap
    (6250, 36), (36, 6250), (8000, 36), (8100, 36), (32, 8100), (36, 8000),
]


def _check_transforms(ny, nx, prec, seed):
    import torch
    from orphics_amd.engine import Engine
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((ny, nx))
    z = rng.standard_normal((ny, nx)) + 1j * rng.standard_normal((ny, nx))
    hcin = rng.standard_normal((ny, nx // 2 + 1)) + 1j * rng.standard_normal((ny, nx // 2 + 1))
    tol = TOL[prec]
    e = Engine(ny, nx, prec)
    assert e.mixed and not e.pow2
    # inputs rounded to the plan's precision first: the reference sees the same values
    x = torch.as_tensor(x, dtype=e.rdt).double().numpy()
    z = torch.as_tensor(z, dtype=e.cdt).to(torch.complex128).numpy()
    hcin = torch.as_tensor(hcin, dtype=e.cdt).to(torch.complex128).numpy()

    def err(got, ref):
        return np.abs(got - ref).max() / np.abs(ref).max()

    k = e.rfft(e.to_real(x))
    errs = {"rfft": err(k.cpu().numpy()[:, :nx // 2 + 1], np.fft.rfft2(x))}
    h = e.hc()
    h[:, :nx // 2 + 1] = torch.as_tensor(hcin, dtype=e.cdt, device=e.device)
    # irfft: numpy's irfft2 drops the imaginary parts of the self-conjugate columns after the column transform, i.e. keeps their
    # Hermitian part, which is the library's convention
    errs["irfft"] = err(e.irfft(h, scale=1.0).cpu().numpy(), np.fft.irfft2(hcin, s=(ny, nx)) * (ny * nx))
    zt = torch.as_tensor(z, dtype=e.cdt, device=e.device)
    errs["cfft"] = err(e.cfft(zt).cpu().numpy(), np.fft.fft2(z))
    errs["icfft"] = err(e.cfft(zt, inverse=True).cpu().numpy(), np.fft.ifft2(z) * (ny * nx))
    bad = {name: v for name, v in errs.items() if not v <= tol}
    assert not bad, (ny, nx, prec, bad)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("ny,nx", SHAPES)
def test_mixed_radix_transforms_match_numpy(ny, nx, prec):
    """rfft / irfft / cfft / inverse cfft of a mixed-radix plan == numpy.fft (float64) at the branch edges listed in SHAPES."""
    _check_transforms(ny, nx, prec, seed=ny * 8191 + nx)


def _mixed_sides(lo, hi):
    out = []
    for n in range(lo, hi + 1, 2):
        m = n
        for p in (2, 3, 5):
            while m % p == 0:
                m //= p
        if m == 1 and n & (n - 1):
            out.append(n)
    return out


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_every_large_mixed_side_transforms(prec):
    """Every side above 5000 that oa_plan_create accepts transforms correctly along both axes (columns: (N, 36); complex and real
    rows: (32, N)): no launch is refused for the LDS budget (float64 sides above 5120 take the in-place stages)."""
    sides = _mixed_sides(5000, 8192)
    assert sides[0] == 5000 and sides[-1] == 8100 and len(sides) == 20
    for n in sides:
        _check_transforms(n, 36, prec, seed=n)
        _check_transforms(32, n, prec, seed=n + 1)
