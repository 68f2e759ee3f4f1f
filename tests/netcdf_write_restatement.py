"""Helper of tests/test_netcdf_write_host.py and tests/test_gpu_netcdf_write.py (no tests here): plain statements of what the netCDF
writers and dbm_chunk_encode's stage (a) compute -- the cutting of a plane into whole chunks, their zero padding and the file's row
order -- and the planes both test files write.  The shuffle itself is tests/netcdf_restatement.py's."""
import numpy as np

from netcdf_restatement import same, shuffle  # noqa: F401

PIXEL = 250.0
BOUND = (-1000.0, 500.0, -1000.0 + 45 * PIXEL, 500.0 + 70 * PIXEL)     # 70 x 45 pixels of 250 m: every coordinate is exact in float64


def bound_of(shape):
    """window_bound of an (H, W) or (1, H, W) plane of 250 m pixels."""
    return (-1000.0, 500.0, -1000.0 + shape[-1] * PIXEL, 500.0 + shape[-2] * PIXEL)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def chunk_bytes(plane, ch, cw, index, y_ascending=False):
    """The unshuffled bytes of chunk `index` (row-major over the chunks) of the float32 (H, W) plane: chunk row r is plane row r0 + r,
    or H - 1 - (r0 + r) in a file whose y ascends; positions beyond the plane are zero bytes; the values are the 32-bit patterns,
    little endian."""
    H, W = plane.shape
    nx = -(-W // cw)
    r0, c0 = (index // nx) * ch, (index % nx) * cw
    words = bits(plane)
    out = np.zeros((ch, cw), dtype="<u4")
    for r in range(ch):
        if r0 + r >= H:
            break
        row = H - 1 - (r0 + r) if y_ascending else r0 + r
        for c in range(min(cw, W - c0)):
            out[r, c] = words[row, c0 + c]
    return out.tobytes()


def noise_plane(H, W, seed=5):
    """Noise with sigma = 300, a constant region, NaNs (one with a payload), both infinities and -0.0."""
    a = np.random.default_rng(seed).normal(0.0, 300.0, (H, W)).astype(np.float32)
    if H > 40 and W > 30:
        a[20:40, 10:30] = -9999.0
    flat = a.reshape(-1)
    if flat.size >= 15:
        flat[7] = np.nan
        a.view(np.uint32).reshape(-1)[9] = 0x7FC12345   # (a view: written into `a`)
        flat[11], flat[12], flat[13] = np.inf, -np.inf, -0.0
    return a


def contents():
    """One 256 x 256 chunk each."""
    r = np.random.default_rng(9)
    noise = r.normal(0.0, 300.0, (256, 256)).astype(np.float32)
    constant = np.full((256, 256), -2000.0, dtype=np.float32)
    half = constant.copy()
    half[128:] = noise[128:]
    ramp = (3.0 * np.arange(256, dtype=np.float32)[None, :] + np.arange(256, dtype=np.float32)[:, None]).astype(np.float32)
    special = noise.copy()
    special[0, :8] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 3.4e38, -1.5]
    special[100:160, 30:200] = np.nan
    special.view(np.uint32)[100:160, 30:200] = 0x7FC00BED
    random_bits = r.integers(0, 1 << 32, (256, 256), dtype=np.uint64).astype(np.uint32).view(np.float32)
    return {"noise": noise, "constant": constant, "half constant": half, "ramp": ramp, "nan inf zero": special, "random bits": random_bits}
