"""-m gpu: dbm_grid_tension_surface, dbm_grid_distance_mask and dbm_grid_to_pixel (reference data_prep.py:409-441) through the C ABI and
through deepbedmap_amd/gridding.py, against the SciPy restatement (tests/surface_restatement.py: Kronecker operator, direct float64
solve; pinned to hand-computed facts in tests/test_surface_host.py).

Surface: |GPU - restatement| <= 1e-3 m.  Derived, not measured: the data stay below 4096 m, where one float32 rounding of the output is
at most 2^-12 = 2.44e-4 m; the conjugate gradients run to |r| <= 1e-12 |b|, which a float64 prototype of the same iteration brought
within 3.3e-8 m of the direct solve; the bound leaves a factor of four.  The worst value seen is printed by every case.
Constraint nodes, the mask, the pixel resampling and the composition are compared BIT FOR BIT."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import surface_restatement as sr  # noqa: E402

pytestmark = pytest.mark.gpu

TOL, MAX_ITER, BOUND = 1e-12, 5000, 1e-3
TILE = (16, 64)   # surface.hip: SURF_TR x SURF_TC

# (shape, constraint density or count, tension): every shape of the issue, and 17 x 65 = one node past the operator's tile in each axis
CASES = [
    ((3, 3), 1, 0.35),
    ((4, 4), 0.5, 0.35),
    ((3, 200), 0.05, 0.35),
    ((200, 3), 0.05, 0.35),
    ((37, 70), 0.08, 0.35),
    ((37, 70), 1, 0.35),
    ((37, 70), 0.08, 0.01),
    ((37, 70), 0.08, 1.0),
    ((67, 133), 0.03, 0.35),
    ((TILE[0] + 1, TILE[1] + 1), 0.08, 0.35),
]


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d

    return d


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def raster(shape, density, seed=11):
    """float32 (H, W): NaN except on the constraint nodes, |z| < 4096 m; density: a fraction of the nodes, or their number"""
    rng = np.random.default_rng(seed + 1000 * shape[0] + shape[1])
    n = shape[0] * shape[1]
    k = density if isinstance(density, int) else max(1, int(round(density * n)))
    d = np.full(n, np.nan, dtype=np.float32)
    d[rng.choice(n, k, replace=False)] = rng.uniform(-4095.0, 4095.0, k).astype(np.float32)
    return d.reshape(shape)


_solved = {}


def solved(shape, density, tension):
    """(data, restatement) of a case, computed once"""
    key = (shape, density, tension)
    if key not in _solved:
        d = raster(shape, density)
        _solved[key] = (d, sr.tension_surface(d, tension))
    return _solved[key]


@pytest.mark.parametrize("shape,density,tension", CASES)
def test_surface_matches_the_direct_solve(dbm, shape, density, tension):
    d, want = solved(shape, density, tension)
    got, info = dbm.tension_surface(d, tension=tension, tol=TOL, max_iter=MAX_ITER)
    k = ~np.isnan(d)
    worst = float(np.abs(got.astype(np.float64) - want).max())
    print(f"surface {shape} density {density} T {tension}: {info['iterations']} iterations, residual {info['residual']:.3e}, "
          f"max |gpu - direct| {worst:.3e} m")
    assert got.dtype == np.float32 and got.shape == shape
    assert info["constraints"] == int(k.sum()) and info["free"] == int((~k).sum())
    assert np.array_equal(bits(got[k]), bits(d[k]))          # constraint nodes come back bit for bit
    assert np.isfinite(got).all()
    assert 0 <= info["iterations"] <= MAX_ITER and info["residual"] <= TOL
    assert worst <= BOUND


def test_one_constraint_is_the_constant_in_zero_iterations(dbm):
    d, _ = solved((3, 3), 1, 0.35)
    got, info = dbm.tension_surface(d, tol=TOL, max_iter=MAX_ITER)
    assert info["iterations"] == 0 and info["residual"] == 0.0
    assert np.array_equal(bits(got), bits(np.full((3, 3), d[~np.isnan(d)][0], dtype=np.float32)))
    big, _ = solved((37, 70), 1, 0.35)
    got, info = dbm.tension_surface(big, tol=TOL, max_iter=MAX_ITER)
    assert info["iterations"] == 0
    assert np.array_equal(bits(got), bits(np.full((37, 70), big[~np.isnan(big)][0], dtype=np.float32)))


def test_two_calls_give_identical_bytes(dbm):
    d, _ = solved((37, 70), 0.08, 0.35)
    a, ia = dbm.tension_surface(d, tol=TOL, max_iter=MAX_ITER)
    b, ib = dbm.tension_surface(d, tol=TOL, max_iter=MAX_ITER)
    assert np.array_equal(bits(a), bits(b)) and ia == ib


def test_default_tolerance_and_resident_input(dbm):
    from deepbedmap_amd.srgan import DeviceArray, to_device

    d, want = solved((67, 133), 0.03, 0.35)
    dev = to_device(d)
    out, info = dbm.tension_surface(dev, download=False)
    assert isinstance(out, DeviceArray) and out.shape == d.shape and info["residual"] <= 1e-9
    assert np.abs(out.get().astype(np.float64) - want).max() <= BOUND   # tol 1e-9 of |b| ~ 1e5: well inside
    assert np.array_equal(bits(dev.get()), bits(d))                      # the input is not touched


def _call_surface(dbm, ddata, H, W, tension, tol, max_iter, dout, info=True):
    from deepbedmap_amd import _lib

    ctx = _lib.default_context()
    buf = np.full(4, -1.0)
    rc = _lib.lib().dbm_grid_tension_surface(ctx.handle, C.c_void_p(ddata) if ddata else None, H, W, tension, tol, max_iter,
                                             C.c_void_p(dout) if dout else None, buf.ctypes.data_as(C.POINTER(C.c_double)) if info else None)
    return rc, buf


def test_not_converged_is_status_10_with_info_and_the_last_iterate(dbm):
    from deepbedmap_amd import _lib
    from deepbedmap_amd.srgan import DeviceArray, to_device

    d, want = solved((37, 70), 0.08, 0.35)
    dev, out = to_device(d), DeviceArray(d.shape)
    rc, info = _call_surface(dbm, dev.ptr, 37, 70, 0.35, TOL, 3, out.ptr)
    assert rc == 10
    assert b"not converged" in _lib.lib().dbm_last_error(_lib.default_context().handle)
    k = ~np.isnan(d)
    assert info[0] == 3 and np.isfinite(info[1]) and info[1] > TOL and info[2] == k.sum() and info[3] == (~k).sum()
    last = out.get()
    assert np.isfinite(last).all() and np.array_equal(bits(last[k]), bits(d[k]))
    with pytest.raises(dbm.DbmError) as err:
        dbm.tension_surface(d, tol=TOL, max_iter=3)
    assert err.value.code == 10
    rc, info = _call_surface(dbm, dev.ptr, 37, 70, 0.35, TOL, MAX_ITER, out.ptr)   # the context is fine afterwards
    assert rc == 0 and np.abs(out.get().astype(np.float64) - want).max() <= BOUND


def test_every_refusal_is_status_1_and_writes_nothing(dbm):
    from deepbedmap_amd import _lib
    from deepbedmap_amd.srgan import DeviceArray, to_device

    d = raster((5, 6), 0.3)
    dev, out = to_device(d), to_device(np.full((5, 6), 7.0, dtype=np.float32))
    ok = dict(H=5, W=6, tension=0.35, tol=1e-9, max_iter=100)
    bad = [dict(H=2, W=15), dict(H=15, W=2), dict(H=65536, W=32768), dict(H=-5), dict(tension=0.0), dict(tension=-0.1), dict(tension=1.0001),
           dict(tension=float("nan")), dict(tol=0.0), dict(tol=1.0), dict(tol=float("nan")), dict(max_iter=0), dict(max_iter=10 ** 6 + 1)]
    for change in bad:
        a = dict(ok, **change)
        rc, _ = _call_surface(dbm, dev.ptr, a["H"], a["W"], a["tension"], a["tol"], a["max_iter"], out.ptr)
        assert rc == 1, change
    assert _call_surface(dbm, None, 5, 6, 0.35, 1e-9, 100, out.ptr)[0] == 1
    assert _call_surface(dbm, dev.ptr, 5, 6, 0.35, 1e-9, 100, None)[0] == 1
    assert _call_surface(dbm, dev.ptr, 5, 6, 0.35, 1e-9, 100, out.ptr, info=False)[0] == 1
    empty = to_device(np.full((5, 6), np.nan, dtype=np.float32))
    assert _call_surface(dbm, empty.ptr, 5, 6, 0.35, 1e-9, 100, out.ptr)[0] == 1
    assert b"no constraint node" in _lib.lib().dbm_last_error(_lib.default_context().handle)
    assert np.array_equal(out.get(), np.full((5, 6), 7.0, dtype=np.float32))
    lib, ctx = _lib.lib(), _lib.default_context()
    for radius in (-1, 33):
        assert lib.dbm_grid_distance_mask(ctx.handle, C.c_void_p(dev.ptr), C.c_void_p(out.ptr), 5, 6, radius) == 1
    assert lib.dbm_grid_distance_mask(ctx.handle, C.c_void_p(dev.ptr), C.c_void_p(dev.ptr), 5, 6, 3) == 1
    assert lib.dbm_grid_distance_mask(ctx.handle, None, C.c_void_p(out.ptr), 5, 6, 3) == 1
    assert lib.dbm_grid_distance_mask(ctx.handle, C.c_void_p(dev.ptr), None, 5, 6, 3) == 1
    small = DeviceArray((4, 5))
    assert lib.dbm_grid_to_pixel(ctx.handle, C.c_void_p(dev.ptr), 1, 6, 0.5, C.c_void_p(small.ptr)) == 1
    assert lib.dbm_grid_to_pixel(ctx.handle, C.c_void_p(dev.ptr), 5, 6, 0.0, C.c_void_p(small.ptr)) == 1
    assert lib.dbm_grid_to_pixel(ctx.handle, C.c_void_p(dev.ptr), 5, 6, 0.5, C.c_void_p(dev.ptr)) == 1
    assert lib.dbm_grid_to_pixel(ctx.handle, None, 5, 6, 0.5, C.c_void_p(small.ptr)) == 1
    ctx.synchronize()
    assert np.array_equal(out.get(), np.full((5, 6), 7.0, dtype=np.float32)) and np.array_equal(bits(dev.get()), bits(d))


@pytest.mark.parametrize("shape", [(41, 90), (5, 7)])
@pytest.mark.parametrize("radius", [0, 3, 32])
def test_mask_matches_the_restatement_bit_for_bit(dbm, shape, radius):
    """data nodes in two corners, on an edge and inside; (5, 7) is smaller than the largest radius"""
    from deepbedmap_amd.srgan import to_device

    H, W = shape
    rng = np.random.default_rng(7)
    data = np.full(shape, np.nan, dtype=np.float32)
    data[0, 0], data[H - 1, W - 1], data[H // 2, 0] = 1.0, -2.0, 0.0
    if H > 20:
        data[H // 3, W // 2] = 5.0
        data[0, W - 1] = np.float32(np.inf)   # not NaN: a data node like any other
    grid = rng.uniform(-4000.0, 4000.0, shape).astype(np.float32)
    grid[1, 1] = np.nan                       # a NaN of the surface stays NaN
    want = sr.distance_mask(grid, data, radius)
    got = dbm.mask_far_from_data(grid, data, radius)
    assert np.array_equal(bits(got), bits(want))
    dgrid = to_device(grid)
    assert dbm.mask_far_from_data(dgrid, to_device(data), radius) is dgrid       # resident: in place
    assert np.array_equal(bits(dgrid.get()), bits(want))
    if radius == 0:
        assert (~np.isnan(got)).sum() == (~np.isnan(data)).sum()
    if radius == 32 and H < 20:
        assert not np.isnan(np.delete(got.ravel(), 1 * W + 1)).any()


@pytest.mark.parametrize("holes", [False, True])
def test_to_pixel_is_grdtrack_at_the_cell_centres_bit_for_bit(dbm, holes):
    rng = np.random.default_rng(23)
    H, W = 19, 70
    yy, xx = np.mgrid[0:H, 0:W]
    grid = (900.0 * np.sin(xx / 5.0) * np.cos(yy / 3.0) + rng.normal(0.0, 40.0, (H, W))).astype(np.float32)
    if holes:
        grid[rng.random((H, W)) < 0.15] = np.nan
        grid[0:3, 0:4] = np.nan
        grid[H - 1, W - 5:] = np.nan
    unit = dbm.GridGeometry(0.0, 0.0, 1.0, 1.0)
    cy, cx = np.mgrid[0:H - 1, 0:W - 1]
    mid = np.stack([cx.ravel() + 0.5, cy.ravel() + 0.5], axis=1)
    z, _ = dbm.grdtrack(mid, grid, unit, interpolation="bicubic", threshold=0.5)
    want = z.astype(np.float32).reshape(H - 1, W - 1)
    got, geometry = dbm.to_pixel_registration(grid, dbm.GridGeometry(-1000.0, 5000.0, 250.0, -250.0))
    assert got.shape == (H - 1, W - 1) and got.dtype == np.float32
    assert np.array_equal(bits(got), bits(want))
    assert geometry == dbm.GridGeometry(-875.0, 4875.0, 250.0, -250.0, "pixel")
    if holes:
        assert np.isnan(got).any() and np.isfinite(got).any()
        soft = sr.to_pixel(grid, 0.5)
        assert np.array_equal(np.isnan(got), np.isnan(soft))
        assert np.nanmax(np.abs(got - soft)) <= 1e-3      # below 4096 m: one float32 rounding (2.44e-4 m) and float64 noise
    else:
        assert np.abs(got - sr.to_pixel(grid)).max() <= 1e-3


def reference_cloud():
    """the 20-point cloud of the reference's xyz_to_grid doctest (data_prep.py:393-396)"""
    return 600.0 * np.random.RandomState(seed=42).rand(60).reshape(20, 3)


def test_xyz_to_grid_is_the_composition_of_its_stages_bit_for_bit(dbm):
    xyz = reference_cloud()
    region = "0/750/0/750"
    got, geometry = dbm.xyz_to_grid(xyz, region, spacing=250)
    assert got.shape == (3, 3) and got.dtype == np.float32
    assert geometry == dbm.GridGeometry(125.0, 625.0, 250.0, -250.0, "pixel")
    medians, g0 = dbm.blockmedian_grid(xyz, region, 250, download=False)
    surface, _ = dbm.tension_surface(medians, tension=0.35, download=False)
    dbm.mask_far_from_data(surface, medians, 3)
    want, g1 = dbm.to_pixel_registration(surface, g0, download=True)
    assert np.array_equal(bits(got), bits(want)) and g1 == geometry
    # ... and it is the restatement's chain: the surfaces differ by at most BOUND, the pixel weights' absolute values sum to 25/16, and
    # the output below 1024 m is rounded to float32 once more (2^-14 m)
    soft = sr.to_pixel(sr.distance_mask(sr.tension_surface(medians.get(), 0.35).astype(np.float32), medians.get(), 3))
    print("xyz_to_grid (rows north to south):\n", got)
    assert np.array_equal(np.isnan(got), np.isnan(soft)) and np.isfinite(got).any()
    assert np.nanmax(np.abs(got - soft)) <= 25.0 / 16.0 * BOUND + 2.0 ** -14
    unmasked, _ = dbm.xyz_to_grid(xyz, region, spacing=250, mask_cell_radius=None)
    assert np.isfinite(unmasked).all()
    resident, _ = dbm.xyz_to_grid(xyz, region, spacing=250, download=False)
    assert np.array_equal(bits(resident.get()), bits(got))


def test_xyz_to_grid_takes_a_device_table(dbm):
    rng = np.random.default_rng(5)
    n = 4000
    track = np.stack([rng.uniform(0.0, 20000.0, n), 6000.0 + 3000.0 * np.sin(np.linspace(0.0, 9.0, n)) + rng.normal(0.0, 60.0, n),
                      rng.uniform(-3000.0, 1500.0, n)], axis=1)
    region = "0/20000/0/12000"
    host, gh = dbm.xyz_to_grid(track, region, spacing=250)
    dev, gd = dbm.xyz_to_grid(dbm.DevicePoints(track), region, spacing=250)
    assert host.shape == (48, 80) and gh == gd
    assert np.array_equal(bits(host), bits(dev))
    assert np.isnan(host).any() and np.isfinite(host).any()     # masked far from the track, filled near it
