"""CPU checks of the tension surface's definition (tests/surface_restatement.py: what dbm_grid_tension_surface, dbm_grid_distance_mask
and dbm_grid_to_pixel compute) against facts that do not come from it -- the interior coefficients worked out by hand, symmetry, null
spaces, the transpose symmetry of the problem, a counted disc -- and of the host-side refusals of deepbedmap_amd/gridding.py and the
status text of the bindings, which need no GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import surface_restatement as sr  # noqa: E402


def test_interior_row_has_the_hand_computed_coefficients():
    """T = 0.35: 20 (1 - T) + 4 T = 14.4 at the node, -(8 (1 - T) + T) = -5.55 at the neighbours, 2 (1 - T) = 1.3 at the diagonals,
    (1 - T) = 0.65 at distance two, nothing else"""
    A = sr.operator(9, 9, 0.35).toarray()
    row = A[4 * 9 + 4].reshape(9, 9)
    want = np.zeros((9, 9))
    want[4, 4] = 14.4
    for dr, dc in ((0, 1), (1, 0), (0, -1), (-1, 0)):
        want[4 + dr, 4 + dc] = -5.55
        want[4 + 2 * dr, 4 + 2 * dc] = 0.65
    for dr, dc in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        want[4 + dr, 4 + dc] = 1.3
    assert np.abs(row - want).max() <= 1e-14


@pytest.mark.parametrize("shape", [(3, 3), (4, 7), (9, 5)])
@pytest.mark.parametrize("T", [0.01, 0.35, 1.0])
def test_operator_is_symmetric_and_annihilates_constants(shape, T):
    H, W = shape
    A = sr.operator(H, W, T)
    assert abs(A - A.T).max() <= 1e-14
    assert np.abs(A @ np.ones(H * W)).max() <= 1e-13


def test_bending_term_annihilates_planes():
    """second differences of a plane vanish: with the gradient term taken out, A (a + b x + c y) = 0, edges and corners included"""
    H, W = 6, 8
    A = sr.operator(H, W, 0.35, gradient_weight=0.0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    plane = 3.0 - 2.0 * xx + 0.5 * yy
    assert np.abs(A @ plane.ravel()).max() <= 1e-12
    assert np.abs(sr.operator(H, W, 0.35) @ plane.ravel()).max() > 0.1   # ... and the gradient term does not


def test_free_block_is_positive_definite_with_one_constraint():
    H, W = 5, 6
    A = sr.operator(H, W, 0.35).toarray()
    free = np.ones(H * W, dtype=bool)
    free[7] = False
    assert np.linalg.eigvalsh(A[free][:, free]).min() > 0.0
    assert abs(np.linalg.eigvalsh(A).min()) <= 1e-12   # the whole operator is only semi-definite (constants)


def test_transposing_the_input_transposes_the_solution():
    rng = np.random.default_rng(3)
    d = np.full((23, 31), np.nan)
    pick = rng.random(d.shape) < 0.08
    d[pick] = rng.uniform(-4000.0, 4000.0, int(pick.sum()))
    u, ut = sr.tension_surface(d, 0.35), sr.tension_surface(d.T.copy(), 0.35)
    assert np.abs(u - ut.T).max() <= 1e-9   # metres; two sparse LU solves of values up to 4096 m
    assert np.array_equal(u[pick], d[pick])


def test_constant_data_give_the_constant():
    d = np.full((6, 7), np.nan)
    d[1, 2] = d[4, 5] = d[0, 0] = -812.5
    assert np.array_equal(sr.tension_surface(d, 0.35), np.full((6, 7), -812.5))
    one = np.full((3, 3), np.nan)
    one[1, 1] = 7.0
    assert np.array_equal(sr.tension_surface(one), np.full((3, 3), 7.0))


def test_mask_of_one_node_at_radius_3_keeps_29_nodes():
    data = np.full((11, 13), np.nan, dtype=np.float32)
    data[5, 6] = 1.0
    grid = np.arange(11 * 13, dtype=np.float32).reshape(11, 13)
    kept = ~np.isnan(sr.distance_mask(grid, data, 3))
    assert kept.sum() == 29 and kept[5, 9] and kept[7, 8] and not kept[8, 8]
    assert (~np.isnan(sr.distance_mask(grid, data, 0))).sum() == 1
    corner = np.full((4, 4), np.nan, dtype=np.float32)
    corner[0, 0] = 1.0
    kept = ~np.isnan(sr.distance_mask(np.zeros((4, 4), dtype=np.float32), corner, 3))
    assert kept.sum() == 11   # the quarter disc: 4 + 3 + 3 + 1 nodes in rows 0..3
    assert not kept[3, 3] and kept[3, 0] and kept[2, 2]


def test_midpoint_sampler_reproduces_cubics_and_follows_the_nan_rule():
    yy, xx = np.mgrid[0:7, 0:8].astype(np.float64)
    g = 2.0 + 0.5 * xx - 1.5 * yy + 0.25 * xx * yy      # bilinear: reproduced exactly, ghost nodes (linear) included
    want = 2.0 + 0.5 * (xx[:-1, :-1] + 0.5) - 1.5 * (yy[:-1, :-1] + 0.5) + 0.25 * (xx[:-1, :-1] + 0.5) * (yy[:-1, :-1] + 0.5)
    assert np.abs(sr.to_pixel(g) - want).max() <= 1e-12
    h = g.copy()
    h[3, 3] = np.nan
    # the hole is one of the four central nodes of the four cells around it: valid weight 1 - (9/16)^2 = 0.684
    loose, strict = sr.to_pixel(h, 0.5), sr.to_pixel(h, 0.7)
    for r, c in ((2, 2), (2, 3), (3, 2), (3, 3)):
        assert np.isfinite(loose[r, c]) and np.isnan(strict[r, c])
    assert np.isfinite(strict[1, 1]) and np.isfinite(strict[4, 4])        # a corner of the stencil: weight (1/16)^2
    assert np.array_equal(loose[0], sr.to_pixel(g)[0])                    # cells whose stencil misses the hole are untouched
    yy2, xx2 = yy[:-1, :-1] + 0.5, xx[:-1, :-1] + 0.5
    cubic = xx ** 3 - 2.0 * yy ** 2 * xx
    inner = (slice(1, -1), slice(1, -1))                                  # at a midpoint the weights (-1, 9, 9, -1) / 16 are exact for cubics
    assert np.abs(sr.to_pixel(cubic)[inner] - (xx2 ** 3 - 2.0 * yy2 ** 2 * xx2)[inner]).max() <= 1e-9


def test_python_refusals_need_no_gpu():
    import deepbedmap_amd as dbm

    z = np.zeros((5, 5), dtype=np.float32)
    for bad in (dict(grid=np.zeros((2, 5))), dict(grid=np.zeros((5, 2))), dict(grid=np.zeros(5)), dict(grid=z, tension=0.0),
                dict(grid=z, tension=1.5), dict(grid=z, tension=float("nan")), dict(grid=z, tol=0.0), dict(grid=z, tol=1.0),
                dict(grid=z, max_iter=0), dict(grid=z, max_iter=10 ** 6 + 1), dict(grid=z, max_iter=2.5)):
        with pytest.raises(ValueError):
            dbm.tension_surface(**bad)
    for radius in (-1, 33, 1.5):
        with pytest.raises(ValueError):
            dbm.mask_far_from_data(z, z.copy(), radius)
    with pytest.raises(ValueError):
        dbm.mask_far_from_data(z, np.zeros((5, 6), dtype=np.float32))
    with pytest.raises(ValueError):
        dbm.mask_far_from_data(z, z)
    geometry = dbm.GridGeometry(0.0, 750.0, 250.0, -250.0)
    with pytest.raises(ValueError):
        dbm.to_pixel_registration(np.zeros((1, 5)), geometry)
    with pytest.raises(ValueError):
        dbm.to_pixel_registration(z, geometry, threshold=0.0)
    with pytest.raises(ValueError):
        dbm.to_pixel_registration(z, dbm.GridGeometry(0.0, 750.0, 250.0, -250.0, "pixel"))
    with pytest.raises(TypeError):
        dbm.to_pixel_registration(z, (0.0, 750.0, 250.0, -250.0))
    with pytest.raises(ValueError):
        dbm.xyz_to_grid(np.zeros((4, 3)), "0/250/0/750")            # 4 x 2 nodes
    with pytest.raises(ValueError):
        dbm.xyz_to_grid(np.zeros((4, 3)), "0/750/0/750", mask_cell_radius=40)
    with pytest.raises(ValueError):
        dbm.xyz_to_grid(np.zeros((4, 3)), "0/750/0/750", tension=0.0)


def test_status_10_is_documented_where_callers_look():
    header = open(os.path.join(ROOT, "include", "dbm.h")).read()
    assert "Status 10" in header and "not converged within max_iter" in header
    import inspect

    from deepbedmap_amd import _lib, gridding

    assert "10 (dbm_grid_tension_surface only)" in inspect.getsource(_lib.DbmError)
    assert "code 10" in gridding.tension_surface.__doc__
    api = open(os.path.join(ROOT, "deepbedmap_amd", "csrc", "api_data.hip")).read()     # (where dbm_grid_tension_surface lives)
    assert "DbmError(10," in api and "out_dev holds the last iterate" in api
