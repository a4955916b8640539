"""Small sphere scenes whose uniform grid has an always-test (large-primitive) list of a chosen length: shared by
tests/test_gpu_large_block.py and tests/test_walk_consts_large_host.py.

A primitive is large when its box diagonal exceeds four times the median diagonal (rtow_grid.h): 150 spheres of radius
0.2 in a slab are the small ones; the ground (radius 1000) and spheres of radius 1.1 to 1.6 are the large ones.  The large
spheres sit at scattered places of the sphere array, so their ids — and their records in the image — are not adjacent.
Importing this module loads no library."""
import numpy as np

import accel_images as ai

MATS = ((ai.MAT_LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, 1.5), (ai.MAT_LAMBERTIAN, (0.8, 0.3, 0.2), 0.0, 1.5),
        (1, (0.7, 0.8, 0.9), 0.1, 1.5), (ai.MAT_DIELECTRIC, (1.0, 1.0, 1.0), 0.0, 1.5))  # (1: metal)
LENGTHS = (0, 1, 3, 4, 5, 7)  # unused, partly used, exactly full, overflowing block
N_SMALL = 150
BIG_AT = ((0.0, 1.3, 0.0), (-3.5, 1.2, 0.5), (3.5, 1.1, -0.5), (1.0, 1.6, -3.5), (-1.5, 1.4, 3.0), (5.5, 1.5, 2.5))


def _small(rng):
    c = rng.uniform([-6.0, 0.2, -6.0], [6.0, 0.2, 6.0], size=(N_SMALL, 3))
    return np.c_[c, np.full(N_SMALL, 0.2)]


def static_scene(n_large, n_moving=0):
    """Geometry with n_large large static spheres (the ground first among them when there is one); the last n_moving
    small spheres move (upwards, by up to half a unit): the scene class with moving spheres, the same large list."""
    rng = np.random.default_rng(100 + n_large)
    small = _small(rng)
    mov = np.zeros((n_moving, 8))
    if n_moving:
        mov[:, 0:3] = small[-n_moving:, 0:3]
        mov[:, 3:6] = small[-n_moving:, 0:3] + np.c_[np.zeros(n_moving), rng.uniform(0.0, 0.5, n_moving), np.zeros(n_moving)]
        mov[:, 6] = 0.2
        small = small[:-n_moving]
    big = [[0.0, -1000.0, 0.0, 1000.0]] + [[x, y, z, y] for x, y, z in BIG_AT]  # (radius = height: they stand on the ground)
    big = np.array(big[:n_large], np.float64).reshape(-1, 4)
    # the large spheres at scattered positions of the array: after every 23rd small sphere
    rows, b = [], 0
    for i, s in enumerate(small):
        if i % 23 == 5 and b < len(big):
            rows.append(big[b])
            b += 1
        rows.append(s)
    rows.extend(big[b:])
    sph = np.array(rows)
    pmat = (1 + np.arange(len(sph) + n_moving) % 3).astype(np.int32)
    pmat[:len(sph)][sph[:, 3] > 100.0] = 0
    return ai.Geometry(sph, mov, np.zeros((0, 9)), pmat, MATS, (13.0, 2.0, 3.0))


def moving_scene():
    """Static ground and one big static sphere, one big MOVING sphere, small static and small moving spheres: the large
    list mixes the classes (the block serves the static head of it, the rest goes through the id section)."""
    rng = np.random.default_rng(77)
    small = _small(rng)
    sph = np.concatenate([small[:40], [[0.0, -1000.0, 0.0, 1000.0]], small[40:100], [[-3.0, 1.2, 1.0, 1.2]]])
    mov = np.zeros((N_SMALL - 100 + 1, 8))
    mov[:-1, 0:3] = small[100:, 0:3]
    mov[:-1, 3:6] = small[100:, 0:3] + np.c_[np.zeros(50), rng.uniform(0.0, 0.5, 50), np.zeros(50)]
    mov[:-1, 6] = 0.2
    mov[-1] = [2.5, 1.3, -1.0, 3.0, 1.3, -1.5, 1.3, 0.0]
    pmat = (1 + np.arange(len(sph) + len(mov)) % 3).astype(np.int32)
    pmat[40] = 0
    return ai.Geometry(sph, mov, np.zeros((0, 9)), pmat, MATS, (13.0, 2.0, 3.0))


def scenes():
    """name -> (Geometry, entries of the large list, entries the block serves)."""
    out = {f"large{n}": (static_scene(n), n, min(n, 4)) for n in LENGTHS}
    # the same lists in the class with moving spheres: the class whose walk takes the head of the list from the block
    out.update({f"moving_large{n}": (static_scene(n, 30), n, min(n, 4)) for n in LENGTHS})
    out["moving_mixed"] = (moving_scene(), 3, 2)
    return out


def block_of_image(blob, n_sph):
    """The large-list words of the host's block as the image says them: (n_large_fast, record offsets, ids) from the
    header (n_large, off_large) and the id section — rtow_walk_consts.h, fill_large_head."""
    P = ai.parse_grid(blob, None)
    ids = np.frombuffer(blob, np.uint32, min(P["n_large"], 4), P["off_large"])
    nf = 0
    while nf < len(ids) and ids[nf] < n_sph:
        nf += 1
    rec = [int(P["off_sph"] + 32 * i) for i in ids[:nf]] + [0] * (4 - nf)
    return nf, rec, [int(i) for i in ids[:nf]] + [0] * (4 - nf)
