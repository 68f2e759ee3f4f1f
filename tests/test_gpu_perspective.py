"""-m gpu: the perspective view of a resident plane (dbm_grid_perspective, dbm_grid_minmax; perspective.hip), DESIGN.md 6o.

The device walks strips of 64, 8 and 1 cells, skips blocks by their maxima and stops behind the visible hit; the host entry walks every
cell the ray's line meets.  Both run the same cell function, so the device's image and ids must equal the host entry's byte for byte
for every plane x view of tests/perspective_restatement.py: that is the check of the skipping.  On the planes up to 37 x 29 the device
is also compared with the NumPy restatement of the rule (no tolerance), and on 150 x 210 its ids go through the verifier.  Planes:
(2, 2); (1, 5) and (5, 1) without cells; (37, 29) with holes, a broken boundary and infinities: five 8-blocks by four, one 64-block;
(150, 210): three 64-blocks by four, the last ones partial.  Images: 24, 96 and 320 pixels wide: 2, 6 and 20 workgroups across."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import perspective_restatement as pr  # noqa: E402
import relief_restatement as rr  # noqa: E402

pytestmark = pytest.mark.gpu

SETTINGS = {"walls": (pr.LEVEL, pr.FACADE, 4), "open-above": (pr.LEVEL_ABOVE, None, 3), "open": (pr.LEVEL, None, 4),
            "walls-above": (pr.LEVEL_ABOVE, pr.FACADE, 3)}
WIDTHS = {(150, 210): 320, (2, 2): 24}


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d

    return d


@pytest.fixture(scope="module")
def resident(dbm):
    cache = {}

    def get(shape, channels):
        if (shape, channels) not in cache:
            drape = pr.drape_of(shape, channels)
            cache[shape, channels] = (dbm.to_device(pr.plane_of(shape)), dbm.DeviceArray(drape.shape, dtype=np.uint8).set(drape))
        return cache[shape, channels]

    return get


def view_of(dbm, view, level):
    return dbm.View(azimuth=view[0], elevation=view[1], level=level, pixel_size=pr.PIXEL_SIZE)


def scene_values(shape, view, width, facade):
    from deepbedmap_amd import perspective

    z = pr.plane_of(shape)
    finite = z[np.isfinite(z)]
    count = finite.size if min(shape) >= 2 else 0
    return perspective.scene_arguments("test", shape[0], shape[1], shape + (3,), np.uint8, view, None, count, float(finite.min()) if count else 0.0,
                                       float(finite.max()) if count else 0.0, width, None, facade, pr.BACKGROUND)[:3]


def cases(shapes):
    out = []
    for shape in shapes:
        for k, view in enumerate(pr.VIEWS):
            names = list(SETTINGS) if (shape, view) == ((37, 29), pr.VIEWS[0]) else (["walls", "open-above"] if shape != (150, 210) else
                                                                                    [["walls", "open-above"][k % 2]])
            out += [pytest.param(shape, view, name, id=f"{shape[0]}x{shape[1]}-A{view[0]}-E{view[1]}-{name}") for name in names]
    return out


@pytest.mark.parametrize("shape,view,setting", cases(pr.SHAPES))
def test_device_equals_the_host_entry(dbm, resident, shape, view, setting):
    level, facade, channels = SETTINGS[setting]
    plane, drape = resident(shape, channels)
    v, width = view_of(dbm, view, level), WIDTHS.get(shape, 96)
    image, ids = dbm.perspective_image(plane, drape, v, width=width, facade=facade, background=pr.BACKGROUND, return_hits=True)
    want, want_ids = dbm.perspective_image_host(pr.plane_of(shape), pr.drape_of(shape, channels), v, width=width, facade=facade,
                                                background=pr.BACKGROUND, return_hits=True)
    assert image.shape == want.shape and image.dtype == np.uint8 and ids.shape == want_ids.shape and ids.dtype == np.int32
    got_ids = ids.get()
    print(f"{want.shape[1]} x {want.shape[0]}: {(got_ids >= 0).sum()} surface, {(got_ids == -2).sum()} wall pixels, "
          f"{(got_ids != want_ids).sum()} ids differ")
    assert np.array_equal(got_ids, want_ids)
    assert np.array_equal(image.get(), want)
    if min(shape) >= 2 and shape != (2, 2):
        assert (got_ids >= 0).any()


@pytest.mark.parametrize("shape,view,setting", cases(pr.SMALL))
def test_device_equals_the_rule(dbm, resident, shape, view, setting):
    level, facade, channels = SETTINGS[setting]
    plane, drape = resident(shape, channels)
    v, width = view_of(dbm, view, level), WIDTHS.get(shape, 96)
    image, ids = dbm.perspective_image(plane, drape, v, width=width, facade=facade, background=pr.BACKGROUND, return_hits=True)
    values, Wo, Ho = scene_values(shape, v, width, facade)
    want, want_ids = pr.rule(pr.plane_of(shape), pr.drape_of(shape, channels), values, Wo, Ho, facade, pr.BACKGROUND)
    assert np.array_equal(ids.get(), want_ids)
    assert np.array_equal(image.get(), want)


@pytest.mark.parametrize("k,view", list(enumerate(pr.VIEWS)))
def test_verifier_accepts_the_device_ids_on_the_large_plane(dbm, resident, k, view):
    shape, width = (150, 210), 160
    level, facade, channels = SETTINGS[["walls", "open-above"][k % 2]]
    plane, drape = resident(shape, channels)
    v = view_of(dbm, view, level)
    _, ids = dbm.perspective_image(plane, drape, v, width=width, facade=facade, background=pr.BACKGROUND, return_hits=True)
    values, Wo, Ho = scene_values(shape, v, width, facade)
    assert ids.shape == (Ho, Wo)
    nbad, failures = pr.verify(pr.plane_of(shape), values, Wo, Ho, ids.get(), facade is not None)
    assert nbad == 0, failures[:5]


def test_grid_minmax_equals_numpy(dbm):
    for shape in pr.SHAPES + [(1, 1), (300, 1000)]:
        z = pr.plane_of(shape)
        finite = z[np.isfinite(z)]
        assert dbm.grid_minmax(dbm.to_device(z)) == (finite.size, float(finite.min()), float(finite.max())), shape
    z = np.full((9, 11), np.nan, dtype=np.float32)
    z[3, 4], z[5, 5] = np.inf, -np.inf
    count, lo, hi = dbm.grid_minmax(dbm.to_device(z))
    assert count == 0 and np.isnan(lo) and np.isnan(hi)
    # a plane without a finite sample renders the background, with or without a facade
    image, ids = dbm.perspective_image(z, np.zeros((9, 11, 3), dtype=np.uint8), dbm.View(pixel_size=250.0), width=40, facade=pr.FACADE,
                                       background=pr.BACKGROUND, return_hits=True)
    assert (ids.get() == -1).all() and (image.get() == np.array(pr.BACKGROUND, dtype=np.uint8)).all()


def test_two_calls_give_identical_bytes(dbm, resident):
    plane, drape = resident((150, 210), 4)
    v = view_of(dbm, pr.VIEWS[0], pr.LEVEL)
    first = dbm.perspective_image(plane, drape, v, width=320, facade=pr.FACADE, return_hits=True)
    second = dbm.perspective_image(plane, drape, v, width=320, facade=pr.FACADE, return_hits=True)
    assert first[0].get().tobytes() == second[0].get().tobytes() and first[1].get().tobytes() == second[1].get().tobytes()
    # scale in place of width, a Raster in place of the plane: its geometry gives the pixel size
    raster = dbm.Raster(plane, dbm.GridGeometry(0.0, 0.0, pr.PIXEL_SIZE, -pr.PIXEL_SIZE))
    a = dbm.perspective_image(raster, drape, dbm.View(), width=None, scale=0.5)
    b = dbm.perspective_image(plane, drape, dbm.View(pixel_size=pr.PIXEL_SIZE), width=None, scale=0.5)
    assert a.shape == b.shape and np.array_equal(a.get(), b.get())
    with pytest.raises(ValueError, match="square"):
        dbm.perspective_image(dbm.Raster(plane, dbm.GridGeometry(0.0, 0.0, 250.0, -500.0)), drape, dbm.View(), width=64)
    with pytest.raises(ValueError, match="pixel_size"):
        dbm.perspective_image(plane, drape, dbm.View(), width=64)
    with pytest.raises(ValueError, match="float32"):
        dbm.perspective_image(dbm.DeviceArray((4, 4), dtype=np.int32), np.zeros((4, 4, 3), dtype=np.uint8), dbm.View(pixel_size=1.0), width=8)


def test_refusals_return_status_1_with_a_message(dbm, resident):
    from deepbedmap_amd import _lib

    ctx = dbm.default_context()
    lib = _lib.lib()
    plane, drape = resident((37, 29), 4)
    out = dbm.DeviceArray((8, 8, 4), ctx, dtype=np.uint8)
    hits = dbm.DeviceArray((8, 8), ctx, dtype=np.int32)
    view = np.array([np.sin(0.3), np.cos(0.3), np.sin(1.0), np.tan(1.0), -1400.0, 0.04, -30.0, 40.0, 1.0])
    rgba = np.array([9, 9, 9, 255], dtype=np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def call(plane_ptr=plane.ptr, H=37, W=29, drape_ptr=drape.ptr, channels=4, view=view, Wo=8, Ho=8, facade=rgba, background=rgba, out_ptr=out.ptr,
             hits_ptr=hits.ptr, handle=ctx.handle):
        return lib.dbm_grid_perspective(handle, C.c_void_p(plane_ptr), H, W, C.c_void_p(drape_ptr), channels, p(view), Wo, Ho, p(facade),
                                        p(background), C.c_void_p(out_ptr), C.c_void_p(hits_ptr))

    def changed(k, value):
        other = view.copy()
        other[k] = value
        return other

    assert call() == 0
    assert call(facade=None, hits_ptr=None) == 0
    bad = [dict(plane_ptr=None), dict(drape_ptr=None), dict(view=None), dict(background=None), dict(out_ptr=None), dict(channels=2), dict(channels=5),
           dict(H=0), dict(H=1 << 16, W=1 << 15), dict(H=(1 << 15) + 2, W=(1 << 15) + 2), dict(Wo=0), dict(Wo=1 << 16, Ho=1 << 15),
           dict(view=changed(2, 0.0)), dict(view=changed(2, -0.5)), dict(view=changed(3, 0.0)), dict(view=changed(8, 0.0)),
           dict(view=changed(8, -1.0)), dict(view=changed(5, 0.0)), dict(view=changed(0, 0.9))]
    bad += [dict(view=changed(k, value)) for k in range(9) for value in (np.nan, np.inf)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert b"dbm_grid_perspective" in lib.dbm_last_error(ctx.handle), kw
    assert call(handle=None) == 1
    stats = np.zeros(3)
    assert lib.dbm_grid_minmax(ctx.handle, None, 37, 29, p(stats)) == 1
    assert lib.dbm_grid_minmax(ctx.handle, C.c_void_p(plane.ptr), 37, 29, None) == 1
    assert lib.dbm_grid_minmax(ctx.handle, C.c_void_p(plane.ptr), 0, 29, p(stats)) == 1
    assert lib.dbm_grid_minmax(ctx.handle, C.c_void_p(plane.ptr), 1 << 16, 1 << 15, p(stats)) == 1
    assert b"dbm_grid_minmax" in lib.dbm_last_error(ctx.handle)
    assert lib.dbm_grid_minmax(None, C.c_void_p(plane.ptr), 37, 29, p(stats)) == 1
    ctx.synchronize()


def test_plot_3d_view_writes_the_view_of_the_relief(dbm, tmp_path):
    """The PNG decodes to `perspective_image` of the plane under its `relief_image` (shaded, reduced once, nodata masked): what
    `plot_3d_view` promises, and through the host entry over the downloaded drape as well."""
    from deepbedmap_amd import relief

    z = pr.plane_of((150, 210)).copy()
    z[40:60, 100:140] = -9999.0
    geometry = dbm.GridGeometry(x0=1000.0, y0=5000.0, dx=250.0, dy=-250.0, registration="pixel")
    raster = dbm.Raster(dbm.to_device(z), geometry, nodata=-9999.0)
    cpt = relief.make_cpt(relief.read_cpt(rr.GOLDEN_CPT), (-4500, 4500))
    path = dbm.plot_3d_view(raster, str(tmp_path / "view.png"), cpt, shading="+d", width=200, reduce=1)
    assert path == str(tmp_path / "view.png") and not os.path.exists(str(tmp_path / "view.pgw"))
    plane, level_geometry = relief.prepared_plane("test", raster, None, 1)
    assert plane.shape == (75, 105) and level_geometry.dx == 500.0
    drape = dbm.relief_image(plane, cpt, shading="+d", channels=4)
    view = dbm.View(azimuth=202.5, elevation=60.0, level=-1400.0, exaggeration=10.0, pixel_size=500.0)
    want, ids = dbm.perspective_image(plane, drape, view, width=200, facade=(128, 128, 128, 255), return_hits=True)
    got = dbm.read_png(path)
    assert got.shape == want.shape and got.shape[1] == 200
    assert np.array_equal(got, want.get())
    ids = ids.get()
    assert (ids >= 0).sum() > 0.3 * ids.size and (ids == -2).any() and (got[ids == -1][:, 3] == 0).all()
    host = dbm.perspective_image_host(plane.get(), drape.get(), view, width=200, facade=(128, 128, 128, 255))
    assert np.array_equal(got, host)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert np.array_equal(np.asarray(im), got)
