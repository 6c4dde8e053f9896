"""numpy restatement of the narrow-band decode's host-checkable rules: the brick
lattice, the active rule, the ordered brick list, the fill, and the set of voxels marching cubes
needs from a dense volume.  A helper of tests/test_band_host.py and tests/test_gpu_band.py, not
a test file.  Everything is evaluated in fp32, as the device does."""
import numpy as np

BRICK = 8


def n_bricks(N):
    return -(-int(N) // BRICK)


def lattice_indices(N):
    """Fine-grid indices min(8b, N - 1), b = 0..nb, of the lattice along one axis."""
    return np.array([min(BRICK * b, int(N) - 1) for b in range(n_bricks(N) + 1)], np.int64)


def lattice_of(vol):
    """The lattice values [.., nb+1, nb+1, nb+1] of a dense volume [.., N, N, N]."""
    ix = lattice_indices(vol.shape[-1])
    return vol[..., ix[:, None, None], ix[None, :, None], ix[None, None, :]]


def corners(coarse):
    """[8, .., nb, nb, nb]: the 8 corner values of every brick, corner q = (dz, dy, dx) bits."""
    nb = coarse.shape[-1] - 1
    out = []
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                out.append(coarse[..., dz:dz + nb, dy:dy + nb, dx:dx + nb])
    return np.stack(out)


def active_rule(coarse, level, band):
    """bool [.., nb, nb, nb] from lattice values [.., nb+1, nb+1, nb+1] (fp32): a brick is
    active when min over its corners of |v - level| <= band, or its corners are not all on one
    side of level (v > level against v <= level), or a corner is not finite."""
    c = corners(np.asarray(coarse, np.float32))
    lv, bd = np.float32(level), np.float32(band)
    with np.errstate(invalid="ignore"):
        near = (np.abs(c - lv) <= bd).any(0)
        above = (c > lv).any(0)
        below = (c <= lv).any(0)
    return near | (above & below) | ~np.isfinite(c).all(0)


def brick_list(active):
    """Ascending global brick ids (shape nb^3 + (bz nb + by) nb + bx) of the active bricks."""
    return np.flatnonzero(np.asarray(active).reshape(-1)).astype(np.int32)


def brick_to_voxels(per_brick, N):
    """Expand a per-brick array [.., nb, nb, nb] to the dense grid [.., N, N, N]."""
    b = np.arange(int(N)) // BRICK
    return per_brick[..., b[:, None, None], b[None, :, None], b[None, None, :]]


def fill(coarse, N):
    """The dense volume in which every voxel holds its brick's corner-0 (lattice) value."""
    nb = n_bricks(N)
    return brick_to_voxels(np.asarray(coarse)[..., :nb, :nb, :nb], N)


def needed_voxels(vol, level):
    """bool [N, N, N]: all 8 voxels of every cell of `vol` whose corners are not all on one
    side of `level`.  Sides as marching cubes takes them (a corner is inside when v < level):
    these are exactly the cells that emit triangles, so a volume equal to `vol` on these voxels
    and with no other mixed cell has the same mesh."""
    inside = np.asarray(vol) < np.float32(level)
    N = vol.shape[0]
    s = [slice(0, N - 1), slice(1, N)]
    cnt = np.zeros((N - 1,) * 3, np.int32)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cnt += inside[s[dz], s[dy], s[dx]]
    mixed = (cnt > 0) & (cnt < 8)
    need = np.zeros((N,) * 3, bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                need[s[dz], s[dy], s[dx]] |= mixed
    return need
