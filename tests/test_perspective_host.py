"""The perspective view without a GPU: the host entry dbm_grid_perspective_host -- the kernel's own cell, wall and colour
functions under a plain traversal -- against the two referees of tests/perspective_restatement.py, the frame, the refusals of the
Python layer and of the host entry, and the declarations.

The rule restatement costs pixels x cells, so it referees the planes up to 37 x 29 (bytes and ids, no tolerance); the verifier referees
every plane, 150 x 210 included.  Widths: 96 pixels for the planes the rule referees, 160 for the large one (the device test renders
320)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import perspective_restatement as pr  # noqa: E402

ROOT = os.path.dirname(HERE)
# (level, facade, drape channels): the reference's plane with a facade; a level above every sample without one
SETTINGS = {"walls": (pr.LEVEL, pr.FACADE, 4), "open-above": (pr.LEVEL_ABOVE, None, 3), "open": (pr.LEVEL, None, 4),
            "walls-above": (pr.LEVEL_ABOVE, pr.FACADE, 3)}


def width_of(shape):
    return {(150, 210): 160, (2, 2): 24}.get(shape, 96)   # (one cell under DEM heights is a spike: few columns, many rows)


@pytest.fixture(scope="module")
def persp():
    from deepbedmap_amd import perspective

    return perspective


@pytest.fixture(scope="module")
def rendered(persp):
    """(image, ids, values, Wo, Ho) of the host entry, once per case"""
    cache = {}

    def get(shape, view, setting):
        key = (shape, view, setting)
        if key not in cache:
            level, facade, channels = SETTINGS[setting]
            z, drape = pr.plane_of(shape), pr.drape_of(shape, channels)
            v = persp.View(azimuth=view[0], elevation=view[1], level=level, pixel_size=pr.PIXEL_SIZE)
            image, ids = persp.perspective_image_host(z, drape, v, width=width_of(shape), facade=facade, background=pr.BACKGROUND, return_hits=True,
                                                      nthreads=4)
            finite = z[np.isfinite(z)]
            count = finite.size if min(shape) >= 2 else 0
            values, Wo, Ho, _, _ = persp.scene_arguments("test", shape[0], shape[1], drape.shape, drape.dtype, v, None, count,
                                                         float(finite.min()) if count else 0.0, float(finite.max()) if count else 0.0,
                                                         width_of(shape), None, facade, pr.BACKGROUND)
            assert image.shape == (Ho, Wo, 4) and ids.shape == (Ho, Wo)
            cache[key] = (image, ids, values, Wo, Ho)
        return cache[key]

    return get


def cases(shapes):
    out = []
    for shape in shapes:
        for k, view in enumerate(pr.VIEWS):
            names = list(SETTINGS) if (shape, view) == ((37, 29), pr.VIEWS[0]) else (["walls", "open-above"] if shape != (150, 210) else
                                                                                    [["walls", "open-above"][k % 2]])
            out += [pytest.param(shape, view, name, id=f"{shape[0]}x{shape[1]}-A{view[0]}-E{view[1]}-{name}") for name in names]
    return out


@pytest.mark.parametrize("shape,view,setting", cases(pr.SMALL))
def test_host_entry_equals_the_rule(rendered, shape, view, setting):
    level, facade, channels = SETTINGS[setting]
    image, ids, values, Wo, Ho = rendered(shape, view, setting)
    want, want_ids = pr.rule(pr.plane_of(shape), pr.drape_of(shape, channels), values, Wo, Ho, facade, pr.BACKGROUND)
    seen = (ids >= 0).sum()
    print(f"{Wo} x {Ho}: {seen} surface pixels, {(ids == -2).sum()} wall pixels, {np.unique(ids[ids >= 0]).size} triangles")
    assert np.array_equal(ids, want_ids)
    assert np.array_equal(image, want)
    if min(shape) < 2:
        assert (ids == -1).all() and (image == np.array(pr.BACKGROUND, dtype=np.uint8)).all()
    else:
        assert seen > 0 or shape == (2, 2)                  # (the spike's walls may hide its one cell)
        if facade is None:
            assert (ids != -2).all()


@pytest.mark.parametrize("shape,view,setting", cases(pr.SHAPES))
def test_verifier_accepts_the_host_entry(rendered, shape, view, setting):
    _, facade, _ = SETTINGS[setting]
    image, ids, values, Wo, Ho = rendered(shape, view, setting)
    nbad, failures = pr.verify(pr.plane_of(shape), values, Wo, Ho, ids, facade is not None)
    assert nbad == 0, failures[:5]


def test_the_verifier_refuses_other_ids(rendered):
    """The referee is not vacuous: ids moved by one pixel, a hidden triangle and an invented miss are all found."""
    shape, view = (37, 29), pr.VIEWS[0]
    image, ids, values, Wo, Ho = rendered(shape, view, "walls")
    z = pr.plane_of(shape)
    shifted = np.roll(ids, 1, axis=1)
    assert pr.verify(z, values, Wo, Ho, shifted, True)[0] > 0.2 * (ids >= 0).sum()
    missed = np.where(ids >= 0, -1, ids)
    assert pr.verify(z, values, Wo, Ho, missed, True)[0] >= 0.9 * (ids >= 0).sum()


def test_a_flat_plane_seen_from_above_is_the_drape(persp):
    """h = 0 everywhere, E = 89, A = 180 (the viewer in the south: north is up, east to the right), one pixel per grid step: pixel
    (i, j) looks at east j + 0.5, north -(i + 0.5) / sin E, so a drape that is linear in the node indices comes back as that ramp."""
    H, W = 5, 7
    z = np.full((H, W), -1400.0, dtype=np.float32)
    r, c = np.mgrid[0:H, 0:W]
    drape = np.stack([10 * c, 10 * r, np.full((H, W), 77)], axis=2).astype(np.uint8)
    view = persp.View(azimuth=180.0, elevation=89.0, level=-1400.0, pixel_size=250.0)
    image, ids = persp.perspective_image_host(z, drape, view, width=None, scale=1.0, return_hits=True)
    sin_e = np.sin(np.radians(89.0))
    assert image.shape == (4, 6, 4)
    j, i = np.meshgrid(np.arange(6), np.arange(4))
    want = np.stack([np.floor(10 * (j + 0.5) + 0.5), np.floor(10 * (i + 0.5) / sin_e + 0.5), np.full((4, 6), 77), np.full((4, 6), 255)], axis=2)
    assert np.array_equal(image, want.astype(np.uint8))
    assert tuple(image[0, 0]) == (5, 5, 77, 255) and tuple(image[0, -1]) == (55, 5, 77, 255) and tuple(image[-1, 0]) == (5, 35, 77, 255)
    assert np.array_equal(ids >> 1, i * (W - 1) + j)          # pixel (i, j) sees cell (i, j)
    # from the north (A = 0) the same scene is turned by half a turn
    turned = persp.perspective_image_host(z, drape, persp.View(azimuth=0.0, elevation=89.0, level=-1400.0, pixel_size=250.0), width=None, scale=1.0)
    assert np.array_equal(turned[:, :, 0], want[::-1, ::-1, 0].astype(np.uint8))


def test_perspective_frame_known_answers(persp):
    cos30 = np.cos(np.radians(30.0))
    south = persp.View(azimuth=180.0, elevation=30.0)
    Wo, Ho, sx0, sy0, step = persp.perspective_frame(5, 7, -2.0, 3.0, south, width=12)
    assert (Wo, Ho) == (12, 13)                                  # x: east 0 .. 6; y: -2 - 2 cos 30 .. 3 cos 30, 6.33 / 0.5
    assert sx0 == 0.0 and sy0 == pytest.approx(3 * cos30, abs=1e-12) and step == 0.5
    assert persp.perspective_frame(5, 7, -2.0, 3.0, south, scale=2.0) == (Wo, Ho, sx0, sy0, step)
    Wo, Ho, sx0, sy0, step = persp.perspective_frame(5, 7, 1.0, 3.0, persp.View(azimuth=0.0, elevation=30.0), width=6)
    assert (Wo, Ho, sx0, step) == (6, 5, -6.0, 1.0)              # heights 0 .. 3: y from 0 to 2 + 3 cos 30 = 4.6
    assert sy0 == pytest.approx(2.0 + 3 * cos30, abs=1e-9)
    east = persp.perspective_frame(5, 7, 0.0, 0.0, persp.View(azimuth=90.0, elevation=89.0), width=4)
    assert east[:2] == (4, 6) and east[2] == -4.0 and east[4] == 1.0   # from the east: screen x = north, -4 .. 0; y = east sin E
    assert persp.perspective_frame(1, 1, 0.0, 0.0, south, width=3) == (3, 3, 0.0, 0.0, 1.0 / 3.0)   # an extent of 0 counts as 1
    assert persp.sincos_degrees(90.0) == (1.0, 0.0) and persp.sincos_degrees(-90.0) == (-1.0, 0.0) and persp.sincos_degrees(540.0) == (0.0, -1.0)


def test_python_refusals(persp, tmp_path):
    import deepbedmap_amd as dbm

    z, drape = pr.plane_of((5, 1)).reshape(1, 5).copy(), pr.drape_of((1, 5), 3)
    view = persp.View(pixel_size=250.0)
    for kw in (dict(elevation=0.5), dict(elevation=89.5), dict(azimuth=float("nan")), dict(azimuth="north"), dict(level=float("inf")),
               dict(exaggeration=0.0), dict(exaggeration=-1.0), dict(pixel_size=0.0), dict(pixel_size=float("nan")), dict(elevation=True)):
        with pytest.raises(ValueError, match="View"):
            persp.View(**kw)
    host = persp.perspective_image_host
    with pytest.raises(ValueError, match="pixel_size"):
        host(z, drape, persp.View(), width=8)
    with pytest.raises(ValueError, match="square"):
        host(z, drape, persp.View(), width=8, geometry=dbm.GridGeometry(0.0, 0.0, 250.0, -500.0))
    assert host(z, drape, persp.View(), width=8, geometry=dbm.GridGeometry(0.0, 0.0, 250.0, -250.0)).shape[1] == 8
    with pytest.raises(ValueError, match="GridGeometry"):
        host(z, drape, view, width=8, geometry=(0, 0, 1, 1))
    with pytest.raises(ValueError, match="View"):
        host(z, drape, (202.5, 60), width=8)
    with pytest.raises(ValueError, match="drape"):
        host(z, drape[:, :4], view, width=8)
    with pytest.raises(ValueError, match="drape"):
        host(z, drape[:, :, :2], view, width=8)
    with pytest.raises(ValueError, match="drape"):
        host(z, drape.astype(np.float32), view, width=8)
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        host(z[None], drape, view, width=8)
    for kw in (dict(width=8, scale=1.0), dict(width=None), dict(width=0), dict(width=2.5), dict(width=None, scale=0.0), dict(width=None, scale=float("inf"))):
        with pytest.raises(ValueError, match="perspective_frame"):
            host(z, drape, view, **kw)
    with pytest.raises(ValueError, match="below 2\\^31"):
        host(z, drape, view, width=None, scale=1e6)
    for kw in (dict(facade=(1, 2, 3)), dict(facade=(1, 2, 3, 256)), dict(background="white"), dict(background=(0, 0, -1, 0))):
        with pytest.raises(ValueError, match="four bytes"):
            host(z, drape, view, width=8, **kw)
    with pytest.raises(ValueError, match="ascending"):
        persp.perspective_frame(5, 5, 2.0, 1.0, view, width=8)
    with pytest.raises(ValueError, match="empty"):
        persp.perspective_frame(0, 5, 0.0, 1.0, view, width=8)
    # plot_3d_view refuses before it touches the device
    cpt = dbm.grey_cpt(-2500.0, 2500.0)
    with pytest.raises(ValueError, match="world file"):
        dbm.plot_3d_view(z, str(tmp_path / "x.png"), cpt, world_file=True, pixel_size=250.0)
    with pytest.raises(ValueError, match="ColorTable"):
        dbm.plot_3d_view(z, str(tmp_path / "x.png"), None, pixel_size=250.0)
    with pytest.raises(ValueError, match="shading"):
        dbm.plot_3d_view(z, str(tmp_path / "x.png"), cpt, shading="+x", pixel_size=250.0)
    with pytest.raises(ValueError, match="elevation"):
        dbm.plot_3d_view(z, str(tmp_path / "x.png"), cpt, elev=90, pixel_size=250.0)


def test_host_entry_refusals_return_status_1_with_a_message(persp):
    from deepbedmap_amd import _lib

    lib = _lib.lib()
    shape = (37, 29)
    z, drape = pr.plane_of(shape), pr.drape_of(shape, 4)
    view = np.array([np.sin(0.3), np.cos(0.3), np.sin(1.0), np.tan(1.0), -1400.0, 0.04, -30.0, 40.0, 1.0])
    out, hits = np.zeros((8, 8, 4), dtype=np.uint8), np.zeros((8, 8), dtype=np.int32)
    rgba = np.array([9, 9, 9, 255], dtype=np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def call(plane=z, H=37, W=29, drape=drape, channels=4, view=view, Wo=8, Ho=8, facade=rgba, background=rgba, out=out, hits=hits):
        return lib.dbm_grid_perspective_host(p(plane), H, W, p(drape), channels, p(view), Wo, Ho, p(facade), p(background), p(out), p(hits), 2)

    def changed(k, value):
        other = view.copy()
        other[k] = value
        return other

    assert call() == 0
    assert call(facade=None, hits=None) == 0
    bad = [dict(plane=None), dict(drape=None), dict(view=None), dict(background=None), dict(out=None), dict(channels=2), dict(channels=5),
           dict(H=0), dict(H=1 << 16, W=1 << 15), dict(H=(1 << 15) + 2, W=(1 << 15) + 2), dict(Wo=0), dict(Wo=1 << 16, Ho=1 << 15),
           dict(view=changed(2, 0.0)), dict(view=changed(2, -0.5)), dict(view=changed(3, 0.0)), dict(view=changed(8, 0.0)),
           dict(view=changed(8, -1.0)), dict(view=changed(5, 0.0)), dict(view=changed(0, 0.9)), dict(view=changed(1, 0.0))]
    bad += [dict(view=changed(k, value)) for k in range(9) for value in (np.nan, np.inf)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert b"dbm_grid_perspective_host" in lib.dbm_last_error(None), kw


def test_entry_points_are_declared_listed_and_exported():
    import deepbedmap_amd as dbm
    from deepbedmap_amd import _lib

    header = open(os.path.join(ROOT, "include", "dbm.h")).read()
    lib = _lib.lib()
    for name in ("dbm_grid_minmax", "dbm_grid_perspective", "dbm_grid_perspective_host"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert header.count("deepbedmap.py:258-295") >= 4          # the section and each of the three entries cite the reference
    for name in ("View", "perspective_frame", "perspective_image", "perspective_image_host", "plot_3d_view"):
        assert hasattr(dbm, name), name
