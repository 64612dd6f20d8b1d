"""Heightfield contacts and height scan OFF the platforms (test infrastructure, shared by tests/test_terrain_contacts.py - the CPU
lane emulator - and tests/test_gpu_terrain_contacts.py - the HIP library): synthetic heightfields, placement tables, and the checks.

Every other parity test starts from a reset, i.e. on the flat centre platform of a tile, where each heightfield lookup returns one
constant and the normal (0, 0, 1).  Here robots are PLACED (load_state) where the bilinear patch is anything but constant - over a
hash-coded field, on sinusoidal waves, mid-slope, across stair risers, tile seams and the grid's edges - and one teacher-forced step
from that shared state is compared with the fp64 oracle:

  (a) helpers.teacher_forced_check, unchanged, plus the contact forces at the bands tests/test_emu_vs_oracle.py gives `cforce`;
  (b) the lookup alone: the oracle evaluates its observation function on the KERNEL's post-step state, so the height-scan columns
      (and base_height_l2's 3 x 3 ray caster) are compared without the step's dynamics in between;
  (c) the family does what it claims (distinct scan values, loaded spheres on tilted patches, two tread heights, lookups outside
      the grid) - asserted on the oracle's side.

The checks' teeth - defective copies of the oracle's terrain sampler in the tested side's place (`DefectiveSampler`) - and the same
placements on the lane program retyped to double (tests/fp64_terrain_families.py) are in the CPU tier.
"""
import functools
import math

import numpy as np

import oracle.spatial as sp
from helpers import SWITCH_EPS, assert_close, switch_mask, teacher_forced_check
from oracle.env import K as REW_KIND
from oracle.env import OracleEnv
from oracle.physics import TerrainSampler
from robot_lab_amd.scene import build_world, load_bundle

A1, GO2W, G1 = (f"RobotLab-Isaac-Velocity-Rough-Unitree-{r}-v0" for r in ("A1", "Go2W", "G1"))
TITA = "RobotLab-Isaac-Velocity-Rough-DDTRobot-Tita-v0"  # the shipped task that gives base_height_l2 a weight (tests/test_gpu_specs.py)

MAX_MASK = 1.0 / 8.0  # at most this share of a family's envs may sit on a switch of the model (helpers.switch_mask)
CFORCE_BANDS = (5e-3, 5e-2)  # rtol, atol [N] of `cforce` in tests/test_emu_vs_oracle.py

# Check (b), per ray:  |got - want| <= LOOKUP_MARGIN * (sensitivity + rounding) * scale, where
#   sensitivity = the fp64 sampler's own change when the query point moves by one fp32 ulp of the root's world x and y (maximum over
#                 the four sign combinations): what ANY fp32 holder of the root position cannot resolve;
#   rounding    = 2^-24 (|z_sensor| + 4 max|corner height| + |value|): half an ulp for each fp32 operation that forms the stored value
#                 z_sensor - h - offset (three lerps on the corner heights, two subtractions).
# The margin is 8 x the worst ratio error / (sensitivity + rounding) of the fp32 numpy restatement of the same lookup (`scan_fp32`: the
# oracle's sampler and ray geometry evaluated in fp32, the ray's WORLD coordinate included), as the project does elsewhere with 8 x the fp32
# reference's error.  Measured over every family, task and kernel shape: profiles/terrain_parity.txt - "fp32 restatement", worst 50.4 (`seams`:
# a lookup that rounds the world coordinate of a RAY, up to four ulps of the root's, steps over a cell edge onto a riser or a box wall that
# one ulp of the root does not reach); the kernels, which turn the root into cell + fraction in fp64, stay below 0.9 of one unit.
LOOKUP_MARGIN = 8.0 * 50.4


# ------------------------------------------------------------------------------------------------ fields
CODED_AMP = 0.05     # [m] |height| of the hash-coded field outside the mesas: cell slopes up to 2, so that a sphere a few centimetres up is clear of
                     # the ground by the model's measure, too ((z - h) nz > r: the distance along the patch normal)
MESA_HEIGHT = 2.5    # [m] blocks of 64 x 64 nodes (3.2 m) every 512 nodes: rays that land on one leave the clip on the low side
MESA = (3, 5)        # a node belongs to a mesa when (ix >> 6) & 7 == 3 and (iy >> 6) & 7 == 5


def _hash01(ix, iy):
    """An integer hash of the node index pair -> [0, 1): asymmetric in (ix, iy), no period along either axis."""
    h = (ix.astype(np.uint64) * np.uint64(73856093)) ^ (iy.astype(np.uint64) * np.uint64(19349663)) ^ np.uint64(0x9E3779B9)
    h &= np.uint64(0xFFFFFFFF)
    for mul in (0x85EBCA6B, 0xC2B2AE35):  # murmur3's finaliser, on 32 bits
        h ^= h >> np.uint64(16)
        h = (h * np.uint64(mul)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h.astype(np.float64) / 4294967296.0


def is_mesa(ix, iy):
    return (((ix >> 6) & 7) == MESA[0]) & (((iy >> 6) & 7) == MESA[1])


def coded_field(nx, ny):
    """`coded`: a hash of (ix, iy) per node in [-CODED_AMP, CODED_AMP] - a lookup that takes a wrong cell, a wrong corner, ix for iy,
    the row stride nx for ny or cell nx - 1 for nx - 2 returns a visibly different height everywhere, the border strip and the last
    row and column included - plus a few mesas of MESA_HEIGHT."""
    ix, iy = np.meshgrid(np.arange(nx, dtype=np.int64), np.arange(ny, dtype=np.int64), indexing="ij")
    h = CODED_AMP * (2.0 * _hash01(ix, iy) - 1.0) + MESA_HEIGHT * is_mesa(ix, iy)
    return np.ascontiguousarray(h, dtype=np.float32)


# (amplitude [m], period along x [nodes], period along y [nodes], phase): wavelengths 1.6 m, 2.4 m, 3.0 m (0 = no dependence on that axis);
# slopes a 2 pi / lambda = 0.32, 0.32, 0.42 - up to 0.8 where they add up -, the x and y gradients differ in size and sign over most of the field
WAVES = ((0.08, 31.7, 0.0, 0.3), (0.12, 0.0, 47.3, 1.1), (0.20, 71.3, -113.9, 2.0))


def waves_field(nx, ny):
    """`waves`: a sum of three sinusoids with incommensurate wavelengths, evaluated at the integer node indices."""
    ix, iy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    h = np.zeros((nx, ny))
    for a, px, py, ph in WAVES:
        h += a * np.sin(2.0 * math.pi * ((ix / px if px else 0.0) + (iy / py if py else 0.0)) + ph)
    return np.ascontiguousarray(h, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _real_world(task):
    desc, extra = load_bundle(task)
    h, to, _ = build_world(desc, extra, 64, 0)
    td = desc.terrain
    return h, to, (td.nx, td.ny, td.hscale, td.x0, td.y0)


@functools.lru_cache(maxsize=None)
def _field(name, nx, ny):
    return coded_field(nx, ny) if name == "coded" else waves_field(nx, ny)


def make_world(task, N, field, mutate=None):
    """(desc, heights, terrain origins): build_world's descriptor fields and origins, the height array replaced for `coded` / `waves`.
    Observation corruption is switched off (check (b) reads the policy row, too; a Spec's corrupting group may run clean, env_spec.h)."""
    desc, _ = load_bundle(task)
    # (build_world generates the terrain anew on every call: once per session.  Every task gets the world of the reference's ROUGH_TERRAINS_CFG as A1
    # Rough's bundle holds it - Tita's own cfg has flat and rough tiles only, no stairs, slopes or boxes to stand on; the tile grid is the same)
    h, to, grid = _real_world(A1)
    td = desc.terrain
    assert (td.num_rows, td.num_cols, td.tile_size, td.border) == (10, 20, 8.0, 20.0) and not td.is_plane
    td.nx, td.ny, td.hscale, td.x0, td.y0 = grid
    desc.task.policy_corrupt = 0
    desc.task.critic_corrupt = 0
    if mutate is not None:
        mutate(desc)
    if field != "real":
        h = _field(field, td.nx, td.ny)
    return desc, h, to


# ------------------------------------------------------------------------------------------------ placements
def row(x, y, yaw=0.0, roll=0.0, pitch=0.0, clear=None, pen=None, fit=None, back=False, lift=0.0, tag="", treads=False, stride=0.0):
    """One env of a placement table.  z: `clear` [m] = airborne, the lowest collision sphere that far above the ground (+ `lift`);
    `stride` [rad]: a robot with a left and a right hip-pitch joint (a biped) has them turned by -+ that much - one foot ahead, one behind: its
    feet, side by side in the default pose, cannot straddle a riser along its heading otherwise;
    `pen` [m] = touching, the lowest sphere that deep in the ground; `fit` = (sx, sy), with `pen`: the robot is also tilted about the
    horizontal axis across that direction until the spheres ahead of the root along it and those behind touch alike (it stands ON a
    slope or a flight of stairs, not with one end in the air)."""
    return dict(x=float(x), y=float(y), yaw=float(yaw), roll=float(roll), pitch=float(pitch), clear=clear, pen=pen, fit=fit, back=back, lift=lift, tag=tag, treads=treads, stride=stride)


def _tile_centre(td, r, c):
    return (r + 0.5) * td.tile_size - td.num_rows * td.tile_size / 2, (c + 0.5) * td.tile_size - td.num_cols * td.tile_size / 2


def _mesa_origin(td):
    """World position of the low corner of the first mesa block and its side."""
    return td.x0 + (MESA[0] << 6) * td.hscale, td.y0 + (MESA[1] << 6) * td.hscale, 64 * td.hscale


def _far_from_mesas(td, x, y, r=1.3):
    gx, gy = (x - td.x0) / td.hscale, (y - td.y0) / td.hscale
    n = r / td.hscale
    for ax in (gx - n, gx + n):
        for ay in (gy - n, gy + n):
            if is_mesa(np.int64(max(ax, 0)), np.int64(max(ay, 0))):
                return False
    return True


CLIP_HIGH, CLIP_LOW = (0, 1, 2, 3), (4, 5, 6, 7)  # the stated envs of `interior`: lifted 1.5 m (every ray past +1) / next to a mesa (rays on it past -1)


def fam_interior(td, N, rng, ora=None):
    rows = []
    mx, my, ms = _mesa_origin(td)
    for i in range(N):
        while True:  # inside the out-of-bounds line (terrain_out_of_bounds would reset the env in the compared step: `edges` goes there)
            x, y = rng.uniform(-1, 1) * (-td.x0 - 3.5), rng.uniform(-1, 1) * (-td.y0 - 3.5)
            if _far_from_mesas(td, x, y):
                break
        yaw, roll, pitch = rng.uniform(0, 2 * math.pi), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)
        if i in CLIP_HIGH:
            rows.append(row(x, y, yaw, roll, pitch, clear=0.05, lift=1.5, tag="clip+"))
        elif i in CLIP_LOW:  # 0.55 m off a mesa's wall, facing it (or with its side to it): the rays that reach over the wall land 2.5 m up
            k = i - CLIP_LOW[0]
            px, py, yw = [(mx - 0.55, my + 1.1, 0.0), (mx + ms + 0.55, my + 2.0, math.pi), (mx + 1.4, my - 0.55, math.pi / 2), (mx + 2.2, my + ms + 0.55, -math.pi / 2)][k]
            rows.append(row(px, py, yw, clear=0.05, tag="clip-"))
        else:
            rows.append(row(x, y, yaw, roll, pitch, clear=0.05))
    return rows


# node indices at which x0 + ix * hscale is an fp32 number (hscale = 13421773 x 2^-28: ix a multiple of 1024 below |x| = 64 m)
LATTICE_NODES = ((1024, 1024), (2048, 3072), (1024, 3072), (2048, 1024))


def fam_lattice(td, N, rng, ora=None):
    """Roots exactly on a grid node, on a cell edge in x only, in y only, and inside a cell; at yaw 0 and the quarter turns the rays (0.1 m = two
    cells apart) land on nodes and edges themselves, ahead of AND behind the base cell (the floorf of a negative offset)."""
    rows, yaws = [], (0.0, math.pi / 2, math.pi, 0.7)
    for k in range(N):
        ix, iy = LATTICE_NODES[(k // 16) % 4]
        fx, fy = ((0.0, 0.37)[(k // 4) % 2], (0.0, 0.61)[(k // 8) % 2])
        x = float(np.float32(td.x0 + (ix + fx) * td.hscale)) if fx else td.x0 + ix * td.hscale
        y = float(np.float32(td.y0 + (iy + fy) * td.hscale)) if fy else td.y0 + iy * td.hscale
        rows.append(row(x, y, yaws[k % 4], clear=0.05, tag=f"fx{fx}fy{fy}"))
    return rows


def fam_edges(td, N, rng, ora=None):
    """For each grid edge a root 0.3 m inside (part of the scan crosses it), 0.3 m and 1 m outside (1 m: every lookup is clamped - the scan's
    half diagonal is 0.94 m); the four corners, (x0, y0) and the far one - largest world coordinates, largest flat index - included.
    Runs with term_out_of_bounds = 0.  Ordered in rounds of sixteen so that any prefix holds every kind."""
    X0, X1, Y0, Y1 = td.x0, -td.x0, td.y0, -td.y0
    rows = []
    along = (0.23, -0.61, 0.47, -0.12)  # position along the edge, as a fraction of its half length
    for k in range(4):
        yaw = 0.4 + 1.3 * k  # never axis aligned: a clamped scan still sees every ray at a y (or x) of its own
        rows += [row(X0 - 1.0, along[k] * Y1, yaw, clear=0.05, tag="out"), row(X1 + 1.0, -along[k] * Y1, yaw + 0.5, clear=0.05, tag="out"),
                 row(along[k] * X1, Y0 - 1.0, yaw + 1.0, clear=0.05, tag="out"), row(-along[k] * X1, Y1 + 1.0, yaw + 1.5, clear=0.05, tag="out")]
        d = (0.0, -0.3, 0.3, 0.0)[k]  # corners: on the corner itself (twice, two headings), 0.3 m inside and 0.3 m outside along the diagonal
        rows += [row(X0 + d, Y0 + d, yaw, clear=0.05, tag="corner"), row(X1 - d, Y1 - d, yaw + 0.5, clear=0.05, tag="corner"),
                 row(X0 + d, Y1 - d, yaw + 1.0, clear=0.05, tag="corner"), row(X1 - d, Y0 + d, yaw + 1.5, clear=0.05, tag="corner")]
        for dist in (0.3, -0.3):  # inside / outside
            rows += [row(X0 + dist, along[k] * Y1, yaw, clear=0.05), row(X1 - dist, -along[k] * Y1, yaw + 0.5, clear=0.05),
                     row(along[k] * X1, Y0 + dist, yaw + 1.0, clear=0.05), row(-along[k] * X1, Y1 - dist, yaw + 1.5, clear=0.05)]
    return rows[:N]


FACES = ((1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0))


def fam_slopes(td, N, rng, ora=None):
    """Mid-slope (2.7 m from the centre: the platform ends at 1.7 m, the slope at 3.75 m) of hf_pyramid_slope and hf_pyramid_slope_inv in the
    hardest row, on each of the four faces, 0.6 m to either side of the face's centre line (off it both gradient components are non-zero),
    at yaw 0, pi / 4 and pi / 2; touching, tilted onto the slope."""
    rows, r = [], td.num_rows - 1
    for k in range(N):
        col = (16, 18, 17, 19)[(k // 4) % 2 + 2 * ((k // 48) % 2)]
        face = FACES[k % 4]
        side = (0.6, -0.6)[(k // 8) % 2]
        yaw = (0.0, math.pi / 4, math.pi / 2)[(k // 16) % 3]
        cx, cy = _tile_centre(td, r, col)
        x, y = cx + 2.7 * face[0] - side * face[1], cy + 2.7 * face[1] + side * face[0]
        rows.append(row(x + rng.uniform(-0.02, 0.02), y + rng.uniform(-0.02, 0.02), yaw, pen=rng.uniform(0.002, 0.006), fit=face))
    return rows


def heads_along(ora):
    """Does this robot straddle a riser with its front and hind feet (heading along the flight) or with its left and right ones (across it)?
    Along, if the spheres it stands on in the default pose reach further along its x axis than along y - the quadrupeds - or if it can put one
    foot ahead (`stride`: a biped with hip-pitch joints); across otherwise (Tita: two wheels side by side)."""
    if any("left_hip_pitch" in str(n) for n in ora.desc.joint_names):
        return True
    ph = ora.phys
    Rw, ow, _ = ph.kinematics(np.zeros((ora.N, 3)), np.tile([1.0, 0.0, 0.0, 0.0], (ora.N, 1)), np.tile(ora.q0, (ora.N, 1)))
    c = np.stack([ow[0, ph.sphere_link[g]] + Rw[0, ph.sphere_link[g]] @ ph.sphere_center[g] for g in range(ph.G)])
    low = c[:, 2] - ph.sphere_radius < (c[:, 2] - ph.sphere_radius).min() + 0.02
    return np.ptp(c[low, 0]) >= np.ptp(c[low, 1])


def fam_stairs(td, N, rng, ora=None):
    """pyramid_stairs and pyramid_stairs_inv in the hardest row (risers 1.5, 1.8 ... 3.0 m from the centre, treads 0.3 m, risers 0.22 m): the
    root ON a riser (the feet straddle that one) or in the middle of a tread (they straddle two, where they are more than a tread apart), on
    the x faces and the y faces; touching, tilted onto the flight.  Every scan (+-0.8 m) covers three risers or more.  (Heading: heads_along.
    A1's left and right feet, 0.26 m apart, cannot stand on treads 0.22 m apart in height however far it rolls.)
    `treads`: no foot AGAINST a riser's face - a one-cell ramp, nz = 0.22.  Measured with such contacts in the table (A1, 32 of 64 envs, four
    seeds): joint-velocity error of the fp32 step 2.0e-3 .. 4.9e-3 against the flat cap of 5e-3, and one env of 128 at 1.22 x its six-twin
    envelope, while the lane program in double agrees with the oracle to 7e-11 on them - round-off of the stiffest contact there is, which
    teacher_forced_check's caps were not sized for; tilted normals in the contact solve are what `slopes` and `waves` are for."""
    rows, r = [], td.num_rows - 1
    along = heads_along(ora)
    for k in range(N):
        col = (1, 5, 2, 6)[(k // 4) % 2 + 2 * ((k // 32) % 2)]
        face = FACES[k % 4]
        d = ((2.4, 2.25, 2.1, 1.95) if along else (2.4, 2.7, 2.1, 1.8))[(k // 8) % 2 + 2 * ((k // 32) % 2)]
        yaw = math.atan2(face[1], face[0]) + (0.0 if along else math.pi / 2) + (0.0, 0.15, -0.15, 0.0)[(k // 16) % 4]
        cx, cy = _tile_centre(td, r, col)
        t = rng.uniform(-0.5, 0.5)  # along the riser
        x, y = cx + d * face[0] - t * face[1] + 0.013, cy + d * face[1] + t * face[0] + 0.013  # (13 mm off the riser line: no foot sphere centred on a cell edge)
        rows.append(row(x, y, yaw, pen=rng.uniform(0.002, 0.006), fit=face, treads=True, stride=0.3 if along else 0.0))
    return rows


def fam_seams(td, N, rng, ora=None):
    """On the real terrain: across the seam between two tile rows, between the stairs-up and the stairs-down columns, between the tile grid
    and the border; off the platform of a `boxes` tile.  Touching.  In rounds of sixteen (four of each kind)."""
    rows, R = [], td.num_rows - 1
    ts = td.tile_size
    for k in range(4):
        yaw = (0.0, math.pi / 2, 0.8, 2.5)[k]
        pen = lambda: rng.uniform(0.002, 0.006)
        # rows 8 | 9 (x = 32 m) on a boxes, a rough, a slope and a stairs column
        xs = R * ts - td.num_rows * ts / 2
        for c in (9, 13, 16, 1):
            rows.append(row(xs + (0.0, 0.1, -0.1, 0.05)[k], _tile_centre(td, R, c)[1] + (0.7, -1.3, 2.1, -2.6)[k], yaw, pen=pen()))
        # stairs up | stairs down (columns 3 | 4, y = -48 m): on the seam and 0.6 m to either side (the scan then reaches the first riser beyond)
        ys = 4 * ts - td.num_cols * ts / 2
        for j in range(4):
            rows.append(row(_tile_centre(td, R - (j % 2), 0)[0] + (-2.2, 0.4, 1.7, -0.9)[k], ys + (0.0, 0.6, -0.6, 0.3)[j], yaw + (math.pi / 2 if j else 0.0), pen=pen()))
        # tile grid | border: x = +40 m (the hardest row's outer rim) and y = +-80 m
        xe, ye = td.num_rows * ts / 2, td.num_cols * ts / 2
        rows += [row(xe + (0.0, -0.2, 0.2, 0.1)[k], _tile_centre(td, R, (9, 13, 16, 18)[k])[1] + 0.9, yaw, pen=pen()),
                 row(xe - 0.15, _tile_centre(td, R, (10, 14, 17, 19)[k])[1] - 1.7, yaw + 1.0, pen=pen()),
                 row(_tile_centre(td, R - k, 19)[0] + 1.1, ye + (0.0, -0.2, 0.2, 0.1)[k], yaw, pen=pen()),
                 row(_tile_centre(td, R - k, 0)[0] - 0.6, -ye + (0.0, 0.2, -0.2, -0.1)[k], yaw + 2.0, pen=pen())]
        # boxes, off the 2 m platform
        for j, (dx, dy) in enumerate(((1.6, 0.3), (-1.3, 1.9), (0.5, -2.4), (-2.8, -1.1))):
            cx, cy = _tile_centre(td, R - (k % 2), 8 + j)
            rows.append(row(cx + dx + 0.11 * k, cy + dy - 0.07 * k, rng.uniform(0, 2 * math.pi), pen=pen()))
    return rows[:N]


ON_BACK = (0, 1, 2, 3, 4, 5)  # the stated envs of `waves`: on their backs, the trunk's spheres carry on a tilted patch


def fam_waves(td, N, rng, ora=None):
    rows = []
    for i in range(N):
        while True:  # seeded random positions; three in four where the waves' gradient under the root is 0.25 or more (nz < 0.97)
            x, y = rng.uniform(-1, 1) * (-td.x0 - 4.0), rng.uniform(-1, 1) * (-td.y0 - 4.0)
            gx, gy = (x - td.x0) / td.hscale, (y - td.y0) / td.hscale
            dx = sum(a * 2 * math.pi / px * math.cos(2 * math.pi * ((gx / px if px else 0.0) + (gy / py if py else 0.0)) + ph) for a, px, py, ph in WAVES if px)
            dy = sum(a * 2 * math.pi / py * math.cos(2 * math.pi * ((gx / px if px else 0.0) + (gy / py if py else 0.0)) + ph) for a, px, py, ph in WAVES if py)
            if i % 4 == 3 or math.hypot(dx, dy) / td.hscale >= 0.25:
                break
        # (on its back the trunk is pressed 1.5 - 3 cm in, as in tests/test_teacher_forced.py: the hips, deeper still, lift a trunk that merely touches
        # off the ground within the step's four substeps)
        rows.append(row(x, y, rng.uniform(0, 2 * math.pi), pen=rng.uniform(0.015, 0.03) if i in ON_BACK else rng.uniform(0.004, 0.008), back=i in ON_BACK))
    return rows


def _no_oob(desc):
    desc.task.term_out_of_bounds = 0


# family -> (field, table builder, descriptor edit, seed)
FAMILIES = dict(interior=("coded", fam_interior, None, 1), lattice=("coded", fam_lattice, None, 2), edges=("coded", fam_edges, _no_oob, 3),
                slopes=("real", fam_slopes, None, 4), stairs=("real", fam_stairs, None, 5), seams=("real", fam_seams, None, 6),
                waves=("waves", fam_waves, None, 7))


def sphere_contacts(ora):
    """World centres [N, G, 3] of the collision spheres in the oracle's current state, terrain height and normal under each, penetration."""
    ph, st = ora.phys, ora.st
    Rw, ow, _ = ph.kinematics(st["root_pos"], st["root_quat"], st["q"])
    cw = np.stack([ow[:, ph.sphere_link[g]] + np.einsum("nij,j->ni", Rw[:, ph.sphere_link[g]], ph.sphere_center[g]) for g in range(ph.G)], 1)
    hz, nrm = ph.terrain.sample(cw[..., 0], cw[..., 1])
    phi = ph.sphere_radius[None] - (cw[..., 2] - hz) * nrm[..., 2]
    return cw, hz, nrm, phi


def trunk_spheres(ora):
    """bool [G]: the collision spheres on the base link or a trunk link (what carries a robot on its back)."""
    m = ora.desc.model
    links = {0} | {int(m.trunk_link[i]) for i in range(m.num_trunk)}
    return np.array([int(l) in links for l in ora.phys.sphere_link])


def _quat_axis(axis, ang):
    q = np.zeros((len(ang), 4))
    q[:, 0] = np.cos(0.5 * ang)
    q[:, 1:] = axis * np.sin(0.5 * ang)[:, None]
    return q


_PLACED = {}


def place(ora, state, rows, key=None):
    """The read_state() dict `state` with the root / joint rows overwritten by the table: default joint positions, zero velocities, z from the
    oracle's own sphere positions (the method of tests/test_emu_vs_oracle.py test_a_hosted_spine_link_carries_the_robot).  `key`: the rows
    depend on the table, the model and the terrain alone - computed once per key and session (the kernel shapes of a task share them)."""
    if key is None or key not in _PLACED:
        _PLACED[key] = _placement(ora, rows)
    rs_rows, q_joint = _PLACED[key]
    out = dict(state)
    rs = np.asarray(state["root_state"], dtype=np.float64).copy()
    rs[:, 0:7], rs[:, 7:13] = rs_rows, 0.0
    out["root_state"] = rs
    out["joint_pos"] = q_joint.copy()
    out["joint_vel"] = np.zeros((ora.N, ora.D))
    return out


def _placement(ora, rows):
    N, st, ph = ora.N, ora.st, ora.phys
    assert len(rows) == N
    get = lambda k, d=0.0: np.array([d if r[k] is None else r[k] for r in rows], dtype=np.float64)
    quat = sp.quat_from_euler_xyz(get("roll"), get("pitch"), get("yaw"))
    back = np.array([r["back"] for r in rows])
    quat = np.where(back[:, None], sp.quat_mul(quat, np.tile([0.0, 1.0, 0.0, 0.0], (N, 1))), quat)  # a half turn about the body's x axis
    touch = np.array([r["pen"] is not None for r in rows])
    depth = np.where(touch, get("pen"), -get("clear"))  # wanted penetration of the lowest sphere (negative: clearance)
    z_hi = float(np.abs(ph.terrain.h).max()) + 3.0
    xy = np.stack([get("x"), get("y")], 1)
    q_joint = np.tile(ora.q0, (N, 1))
    names = [str(n) for n in ora.desc.joint_names]
    for sign, side in ((-1.0, "left_hip_pitch"), (1.0, "right_hip_pitch")):
        for j, n in enumerate(names):
            if side in n:
                q_joint[:, j] += sign * get("stride")
    st["q"] = q_joint

    def drops(q, xy):
        """how far every sphere can come down from z_hi until it is `depth` deep, and where it sits relative to the root"""
        st["root_pos"], st["root_quat"] = np.concatenate([xy, np.full((N, 1), z_hi)], 1), q
        cw, hz, nrm, _ = sphere_contacts(ora)
        return (cw[..., 2] - hz) - (ph.sphere_radius[None] - depth[:, None]) / nrm[..., 2], cw[..., :2] - xy[:, None]

    fit = np.array([r["fit"] is not None for r in rows])
    s = np.array([r["fit"] if r["fit"] is not None else (1.0, 0.0) for r in rows], dtype=np.float64)
    axis = np.stack([-s[:, 1], s[:, 0], np.zeros(N)], 1)  # z x s: a positive angle lowers the end ahead of the root along s
    trunk = trunk_spheres(ora)
    # (the tilt turns the robot about the point on the ground under its root, a standing height `hr` below it - about the root itself the
    # feet would swing back across the risers they are meant to straddle: the root moves ahead by hr sin(angle))
    hr = float(ora.desc.model.default_root_pos[2])

    def solve(xy0):
        """(quaternion, root x y, root z, bool: not a placement - see below) for the table's roots at xy0"""
        ang, jumped = np.zeros(N), np.zeros(N, dtype=bool)
        if fit.any():
            def f(a):  # drop of the spheres ahead of the pivot - drop of those behind: falls as the angle grows
                dz, rel = drops(sp.quat_mul(_quat_axis(axis, a), quat), xy0 + (hr * np.sin(a))[:, None] * s)
                ahead = np.einsum("ngi,ni->ng", rel, s) + (hr * np.sin(a))[:, None] > 0.0
                return np.where(ahead, dz, np.inf).min(axis=1) - np.where(~ahead, dz, np.inf).min(axis=1)

            # on stairs f is not monotone (a foot crosses a riser as the robot leans): the sign change nearest to level on a grid of 2.5 degree
            # steps, then bisection inside that bracket; no sign change within +-0.9 rad = the robot stays level
            grid = np.linspace(-0.9, 0.9, 41)
            fg = np.stack([f(np.full(N, a)) for a in grid], 1)
            cross = (fg[:, :-1] > 0.0) & (fg[:, 1:] <= 0.0) & np.isfinite(fg[:, :-1]) & np.isfinite(fg[:, 1:])
            cost = np.where(cross, np.abs(0.5 * (grid[:-1] + grid[1:]))[None], np.inf)
            j = cost.argmin(axis=1)
            found = np.isfinite(cost.min(axis=1)) & fit
            lo, hi = grid[j], grid[j + 1]
            for _ in range(22):
                mid = 0.5 * (lo + hi)
                fm = f(mid)
                lo, hi = np.where(fm > 0.0, mid, lo), np.where(fm > 0.0, hi, mid)
            ang = np.where(found, 0.5 * (lo + hi), 0.0)
            # (the model's penetration is measured along the patch normal, which JUMPS at a cell edge: where the bracket holds such a jump
            # and no root, the bisection ends with a sphere exactly on the edge and centimetres deep - not a placement)
            jumped = found & ~(np.abs(f(ang)) < 1e-4)
        q = sp.quat_mul(_quat_axis(axis, ang), quat)
        xy1 = xy0 + (hr * np.sin(ang))[:, None] * s
        dz, _ = drops(q, xy1)
        if back.any() and trunk.any():  # on its back: the lowest sphere of the TRUNK body is `pen` deep (a hip or thigh sphere may sit deeper)
            dz = np.where(back[:, None] & ~trunk[None], np.inf, dz)
        z = z_hi - dz.min(axis=1)
        st["root_pos"], st["root_quat"] = np.concatenate([xy1, z[:, None]], 1), q
        _, _, nrm, phi = sphere_contacts(ora)
        return q, xy1, z, (treads & ((phi > -1e-3) & (nrm[..., 2] < 0.7)).any(axis=1)) | jumped

    # `treads`: the feet stand ON the treads to either side of a riser, not against the riser's face (a one-cell ramp, nz = 0.22).  A root
    # whose placement fails - a foot on a riser's face, or no level-footed tilt (above) - is moved along the flight in steps of 25 mm, by
    # up to 0.2 m; if nothing helps the robot stays level
    treads = np.array([r["treads"] for r in rows])
    q_fin, xy_fin, z, todo = solve(xy)
    for d in [sg * 0.025 * i for i in range(1, 9) for sg in (1, -1)]:
        if not todo.any():
            break
        q2, xy2, z2, bad2 = solve(xy + d * s)
        take = todo & ~bad2
        q_fin, xy_fin, z = np.where(take[:, None], q2, q_fin), np.where(take[:, None], xy2, xy_fin), np.where(take, z2, z)
        todo &= bad2
    if todo.any():
        fit = fit & ~todo
        q2, xy2, z2, _ = solve(xy)
        q_fin, xy_fin, z = np.where(todo[:, None], q2, q_fin), np.where(todo[:, None], xy2, xy_fin), np.where(todo, z2, z)
    quat, xy, z = q_fin, xy_fin, z + get("lift")
    return np.concatenate([xy, z[:, None], quat], 1), q_joint


# ------------------------------------------------------------------------------------------------ the two tested sides
STATE_BUFFERS = ("ROOT_STATE", "JOINT_POS", "JOINT_VEL", "ACTION", "GAINS", "CONTACT_TIMERS", "TASK_STATE", "ENV_ORIGIN")


class Driver:
    """A NativeEnv behind the C-ABI - the CPU lane emulator (host pointers) or the HIP library (device pointers) - with the state
    exchange of helpers.emu_read_state / emu_load_state and the outputs teacher_forced_check takes."""

    def __init__(self, desc, heights, origins, N, seed, lib_path=None, gpu=False):
        from robot_lab_amd.capi import NativeEnv

        self.N, self.gpu, self.D = N, gpu, desc.model.num_dof
        self.nat = NativeEnv(desc, heights, origins, None, N, seed, 0, lib_path)
        self._views = {}
        for name in ("CONTACT_FORCE",):  # an inspection view: filled by the steps after the first request
            self.view(name)

    def view(self, name):
        if name not in self._views:
            p, shp, dt = self.nat.buffer(name)
            if self.gpu:
                import torch

                from robot_lab_amd.env import _DevView

                self._views[name] = torch.as_tensor(_DevView(p, shp, dt, self.nat), device="cuda:0")
            else:
                from helpers import host_view

                self._views[name] = host_view(self.nat, name)
        return self._views[name]

    def get(self, name):
        v = self.view(name)
        return v.cpu().numpy().copy() if self.gpu else v.copy()

    def put(self, name, a, cols=None):
        v = self.view(name)
        if cols is not None:
            v = v[:, :cols]
        if self.gpu:
            import torch

            v.copy_(torch.as_tensor(np.ascontiguousarray(a)).to(v.dtype).reshape(v.shape))
        else:
            v[...] = np.asarray(a, dtype=v.dtype).reshape(v.shape)

    def reset(self):
        self.nat.reset()

    def step(self, a):
        from robot_lab_amd.desc import REAL_NP

        a = np.ascontiguousarray(a, dtype=REAL_NP)
        if self.gpu:
            import torch

            t = torch.from_numpy(a).cuda()
            self.nat.step(t.data_ptr())
            torch.cuda.synchronize()
        else:
            self.nat.step(a.ctypes.data)

    def read_state(self):
        self.nat.export_state()
        out = {k.lower(): self.get(k) for k in STATE_BUFFERS}
        out["episode_length"] = self.get("EPISODE_LENGTH")
        out["episode_sums"] = self.get("EPISODE_SUMS")[:, : self.N]
        out["terrain_level"] = self.get("TERRAIN_LEVEL")
        out["step_count"] = self.nat.step_count
        return out

    def load_state(self, s):
        self.nat.export_state()
        for k in STATE_BUFFERS:
            self.put(k, s[k.lower()])
        self.put("EPISODE_LENGTH", s["episode_length"])
        self.put("EPISODE_SUMS", s["episode_sums"], cols=self.N)
        self.put("TERRAIN_LEVEL", s["terrain_level"])
        self.nat.step_count = int(s["step_count"])
        self.nat.commit_state()

    def outputs(self):
        got = self.read_state()
        slot = self.nat.obs_slot()
        got.update(reward=self.get("REWARD"), reward_terms=self.get("REWARD_TERMS")[:, : self.N],
                   done=self.get("TERMINATED").astype(bool) | self.get("TIME_OUT").astype(bool),
                   obs_policy=self.get("OBS_POLICY_RING")[slot, : self.N], obs_critic=self.get("OBS_CRITIC_RING")[slot, : self.N],
                   contact_force=self.get("CONTACT_FORCE"))
        return got

    def close(self):
        self._views = {}
        self.nat.close()


class OracleDriver:
    """An OracleEnv in the place of the tested side (check (d): a DEFECTIVE terrain sampler on this side, the sound one on the other).
    Its state is exchanged as fp32, like a kernel's."""

    def __init__(self, ora):
        self.ora, self.N, self.D = ora, ora.N, ora.D

    def reset(self):
        self.ora.reset()

    def step(self, a):
        self.obs = self.ora.step(a)

    def read_state(self):
        s = self.ora.read_state()
        return {k: (np.asarray(v, dtype=np.float32) if np.asarray(v).dtype == np.float64 else v) for k, v in s.items()}

    def load_state(self, s):
        self.ora.load_state(s)

    def outputs(self):
        o = self.ora
        got = self.read_state()
        got.update(reward=o.reward.copy(), reward_terms=o.reward_terms.copy(), done=(o.terminated | o.time_outs).copy(),
                   obs_policy=self.obs[0].astype(np.float32), obs_critic=self.obs[1].astype(np.float32), contact_force=o.contact_force.copy())
        return got

    def close(self):
        pass


# ------------------------------------------------------------------------------------------------ check (b): the lookup alone
def _patch(td, h, x, y, dtype):
    """TerrainSampler.sample's height in `dtype` arithmetic, and the largest |corner height| of the cell."""
    f = dtype
    x0, y0, hs = f(td.x0), f(td.y0), f(td.hscale)
    gx, gy = (x.astype(f) - x0) / hs, (y.astype(f) - y0) / hs
    ix = np.clip(np.floor(gx), 0, td.nx - 2).astype(np.int64)
    iy = np.clip(np.floor(gy), 0, td.ny - 2).astype(np.int64)
    fx, fy = np.clip(gx - ix.astype(f), f(0), f(1)), np.clip(gy - iy.astype(f), f(0), f(1))
    hh = h.astype(f)
    h00, h10, h01, h11 = hh[ix, iy], hh[ix + 1, iy], hh[ix, iy + 1], hh[ix + 1, iy + 1]
    hx0, hx1 = h00 + fx * (h10 - h00), h01 + fx * (h11 - h01)
    return hx0 + fy * (hx1 - hx0), np.max(np.abs([h00, h10, h01, h11]), axis=0)


def _ray_unit(ora, wx, wy, z_sensor, offset):
    """(value, sensitivity + rounding) per ray: see LOOKUP_MARGIN."""
    samp, td = ora.phys.terrain, ora.desc.terrain
    rp = np.asarray(ora.st["root_pos"], dtype=np.float64)
    ux = np.spacing(np.abs(rp[:, 0]).astype(np.float32)).astype(np.float64)[:, None]
    uy = np.spacing(np.abs(rp[:, 1]).astype(np.float32)).astype(np.float64)[:, None]
    h, _ = samp.sample(wx, wy)
    sens = np.zeros_like(h)
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            sens = np.maximum(sens, np.abs(samp.sample(wx + sx * ux, wy + sy * uy)[0] - h))
    _, hc = _patch(td, samp.h, wx, wy, np.float64)
    v = z_sensor - h - offset
    return h, v, sens + 2.0 ** -24 * (np.abs(z_sensor) + 4.0 * hc + np.abs(v))


def scan_fp32(ora):
    """The fp32 numpy restatement of the height-scan lookup in the oracle's current state: ray geometry, grid transform and bilinear patch of
    oracle/env.py height_scan / oracle/physics.py TerrainSampler with every operation in fp32 (the ray's WORLD coordinate included)."""
    f = np.float32
    t, td = ora.desc.task, ora.desc.terrain
    wx, wy, z = ora.scan_points()
    p0x, p0y = wx[:, t.scan_nx * (t.scan_ny // 2) + t.scan_nx // 2], wy[:, t.scan_nx * (t.scan_ny // 2) + t.scan_nx // 2]  # the centre ray = the sensor
    d0x, d0y = wx[:, t.scan_nx * (t.scan_ny // 2) + t.scan_nx // 2 + 1] - p0x, wy[:, t.scan_nx * (t.scan_ny // 2) + t.scan_nx // 2 + 1] - p0y
    nrm = np.hypot(d0x, d0y)
    c, s = (d0x / nrm).astype(f)[:, None], (d0y / nrm).astype(f)[:, None]
    xs = ((np.arange(t.scan_nx) - (t.scan_nx - 1) / 2).astype(f) * f(t.scan_res))
    ys = ((np.arange(t.scan_ny) - (t.scan_ny - 1) / 2).astype(f) * f(t.scan_res))
    gx, gy = np.meshgrid(xs, ys, indexing="xy")
    lx, ly = gx.reshape(-1)[None], gy.reshape(-1)[None]
    x32 = p0x.astype(f)[:, None] + c * lx - s * ly
    y32 = p0y.astype(f)[:, None] + s * lx + c * ly
    h32, _ = _patch(td, ora.phys.terrain.h, x32, y32, f)
    return z.astype(f) - h32 - f(t.scan_offset)


def _scan_columns(desc, group):
    """(first column, count, ObsTerm) of the height scan in observation group 0 / 1, or None."""
    t = desc.task
    terms, n = ((t.policy, t.n_policy), (t.critic, t.n_critic))[group]
    off, D = 0, desc.model.num_dof
    for i in range(n):
        k = terms[i].kind
        w = 3 if k <= 3 else t.scan_nx * t.scan_ny if k == 7 else D
        if k == 7:
            return off, w, terms[i]
        off += w
    return None


def check_lookup(ora, got, label=""):
    """Check (b).  The oracle adopts the tested side's post-step state `got` and evaluates its observation function there; returns the
    report dict(ratio = worst |err| / (sensitivity + rounding) of the tested side, ratio_fp32 = the same of the fp32 restatement, ...)."""
    t = ora.desc.task
    ora.load_state(got)
    wx, wy, z = ora.scan_points()
    h, v, unit = _ray_unit(ora, wx, wy, z, float(t.scan_offset))
    rep = dict(ratio=0.0, ratio_fp32=float((np.abs(scan_fp32(ora).astype(np.float64) - v) / unit).max()), clipped_lo=0, clipped_hi=0, rays=0)
    bad = []
    for g, key in enumerate(("obs_policy", "obs_critic")):
        sc = _scan_columns(ora.desc, g)
        if sc is None:
            continue
        off, w, term = sc
        lo, hi, scale = float(term.clip_lo), float(term.clip_hi), float(term.scale)
        gv = np.asarray(got[key], dtype=np.float64)[:, off:off + w]
        want = np.clip(v, lo, hi) * scale
        tol = LOOKUP_MARGIN * unit * abs(scale)
        err = np.abs(gv - want)
        inside = (v > lo) & (v < hi)
        rep["ratio"] = max(rep["ratio"], float((err / (unit * abs(scale)))[inside].max()) if inside.any() else 0.0)
        rep["rays"] += int(inside.sum())
        if (err > tol).any():
            i, r = np.unravel_index(np.argmax(err / tol), err.shape)
            bad.append(f"{key}: {int((err > tol).sum())} rays outside {LOOKUP_MARGIN:g} x (sensitivity + rounding); worst env {i} ray {r}: got {gv[i, r]:.7f} want {want[i, r]:.7f} tol {tol[i, r]:.2e}")
        # clipped entries equal the clip value exactly (where the oracle's value is past the bound by more than the tolerance)
        for bound, past, name in ((lo, v < lo - tol, "clipped_lo"), (hi, v > hi + tol, "clipped_hi")):
            rep[name] += int(past.sum())
            exact = float(np.float32(bound) * np.float32(scale))
            if (gv[past] != exact).any():
                bad.append(f"{key}: {int((gv[past] != exact).sum())} entries past the clip at {bound} are not exactly {exact}")
    # base_height_l2 with its 3 x 3 ray caster (rewards.py:616-644): f = (z - target - mean hit height)^2 x gate, on the post-step pose of an env
    # that was not reset (the reward is computed before the resets; the push event changes velocities only)
    for i in range(t.n_rewards):
        rt = t.rewards[i]
        if rt.kind != REW_KIND["base_height_l2"] or float(rt.weight) == 0.0 or float(rt.p[1]) <= 0.5:
            continue
        bx, by = ora.base_scan_points()
        zr = ora.st["root_pos"][:, 2:3]
        hb, _, ub = _ray_unit(ora, bx, by, zr, 0.0)
        gate = np.clip(-ora.derived()["projected_gravity_b"][:, 2], 0.0, 0.7) / 0.7
        d = zr[:, 0] - float(rt.p[0]) - hb.mean(axis=1)
        k = gate * abs(float(rt.weight)) * ora.step_dt
        want = d * d * gate * float(rt.weight) * ora.step_dt
        # d f = 2 |d| d(mean): the rays' units averaged; + 16 half-ulps of the term for the ~8 fp32 operations after the mean (gate, square, weight, dt)
        tol = LOOKUP_MARGIN * 2.0 * np.abs(d) * ub.mean(axis=1) * k + 16.0 * 2.0 ** -24 * np.abs(want) + 1e-12
        live = ~np.asarray(got["done"], dtype=bool)
        err = np.abs(np.asarray(got["reward_terms"], dtype=np.float64)[i] - want)
        rep["base_height_ratio"] = float((err / tol)[live].max() * LOOKUP_MARGIN)
        if (err > tol)[live].any():
            e = int(np.argmax(np.where(live, err / tol, 0.0)))
            bad.append(f"base_height_l2: env {e} got {got['reward_terms'][i][e]:.7e} want {want[e]:.7e} tol {tol[e]:.1e}")
    assert not bad, f"check (b) {label}: " + "; ".join(bad) + f"\nreport: {rep}"
    return rep


# ------------------------------------------------------------------------------------------------ check (c): the family's claims
def check_claims(family, ora, state, rows, peak):
    """Asserted on the oracle's side: `state` the shared state, `peak` [N, B] the largest contact force on each body over the substeps whose
    forces the oracle keeps (the contact sensor's history: the last three of the step's four; zero for an env the step reset)."""
    N, td = ora.N, ora.desc.terrain
    ora.load_state(state)
    tag = np.array([r["tag"] for r in rows])
    info = {}
    if family in ("interior", "lattice", "edges"):
        wx, wy, z = ora.scan_points()
        h, _ = ora.phys.terrain.sample(wx, wy)
        v = z - h - float(ora.desc.task.scan_offset)
        distinct = np.array([len(np.unique(np.round(h[i], 7))) for i in range(N)])
        assert (distinct > 20).all(), f"{family}: scan rows with <= 20 distinct heights: envs {np.nonzero(distinct <= 20)[0]} ({distinct.min()})"
        assert peak.max() == 0.0, f"{family}: airborne by construction, but the oracle has contact forces"
        sc = _scan_columns(ora.desc, 1)[2]
        inside = ((v > sc.clip_lo) & (v < sc.clip_hi)).all(axis=1)
        info["envs_inside_clip"] = int(inside.sum())
        if family == "interior":
            assert (v[list(CLIP_HIGH)] > sc.clip_hi).all() and all((v[i] < sc.clip_lo).sum() >= 10 for i in CLIP_LOW), "interior: the stated envs do not leave the clip on both sides"
            assert inside.sum() >= N - len(CLIP_HIGH) - len(CLIP_LOW) - 2, f"interior: only {inside.sum()} of {N} envs stay inside the clip"
        if family == "edges":
            gx, gy = (wx - td.x0) / td.hscale, (wy - td.y0) / td.hscale
            outside = ((gx < 0) | (gx > td.nx - 1) | (gy < 0) | (gy > td.ny - 1)).all(axis=1)
            assert outside[tag == "out"].all() and (tag == "out").sum() >= N // 8, "edges: a root 1 m outside has lookups inside the grid"
            far = ((gx > td.nx - 1) & (gy > td.ny - 1)).any(axis=1)
            assert far.any() and ((gx < 0) & (gy < 0)).any(), "edges: no ray beyond the corner (x0, y0) / the far corner"
            info["envs_all_outside"] = int(outside.sum())
    else:
        cw, hz, nrm, phi = sphere_contacts(ora)
        body = np.asarray(ora.phys.sphere_body)
        fb = peak[:, body]  # [N, G]: the force on the body each sphere belongs to
        if family in ("slopes", "waves"):
            tilted = (phi > 0.0) & (nrm[..., 2] < 0.98) & (fb > 20.0)
            assert tilted.any(axis=1).sum() >= N // 2, f"{family}: only {tilted.any(axis=1).sum()} of {N} envs carry > 20 N on a patch with nz < 0.98"
            nx_, ny_ = nrm[..., 0][tilted], nrm[..., 1][tilted]
            assert (nx_ > 0.02).any() and (nx_ < -0.02).any() and (ny_ > 0.02).any() and (ny_ < -0.02).any(), f"{family}: the loaded patches do not tilt both ways in x and y"
            info["envs_loaded_on_tilt"] = int(tilted.any(axis=1).sum())
            if family == "waves":  # on their backs: a sphere of the trunk body is in the ground, on a tilted patch for some
                ts = trunk_spheres(ora)
                trunk = ((phi > 0.0) & ts[None]).any(axis=1)
                assert trunk[list(ON_BACK)].all(), "waves: an env on its back does not rest on its trunk"
                info["on_back_trunk_tilted"] = int(((phi > 0.0) & ts[None] & (nrm[..., 2] < 0.98)).any(axis=1)[list(ON_BACK)].sum())
                info["on_back_trunk_force"] = [round(float(x), 1) for x in np.where(ts[None], fb, 0.0).max(axis=1)[list(ON_BACK)]]
        if family == "stairs":
            two = np.array([np.ptp(hz[i][phi[i] > 0.0]) > 0.04 if (phi[i] > 0.0).any() else False for i in range(N)])
            assert two.sum() >= N // 2, f"stairs: only {two.sum()} of {N} envs touch two different tread heights"
            wx, wy, _ = ora.scan_points()
            levels = np.array([len(np.unique(np.round(ora.phys.terrain.sample(wx[i], wy[i])[0] / 0.04))) for i in range(N)])
            assert (levels >= 4).sum() >= N // 2, "stairs: the scans do not cover three risers"
            info["envs_on_two_treads"] = int(two.sum())
        if family == "seams":
            touching = (phi > 0.0).any(axis=1)
            assert touching.all(), "seams: an env does not touch"
    return info


# ------------------------------------------------------------------------------------------------ one case
def oracle_for(desc, h, to, N, seed, sampler=None):
    ora = OracleEnv(desc, h, to, N, seed, None)
    if sampler is not None:
        ora.phys.terrain = sampler
    return ora


def run_case(family, drv, ora, rng_seed=0, checks=("a", "b", "c"), n_twins=6, key=None):
    """reset, two warm-up steps (actions and timers live), read_state, overwrite the root / joint rows from the family's table, load_state,
    read_state again (the shared state is the fp32 one the tested side holds), ONE step on both sides, the checks.  Returns the report."""
    N = ora.N
    field, build, _, seed = FAMILIES[family]
    rows = build(ora.desc.terrain, N, np.random.default_rng(seed), ora)
    rng = np.random.default_rng(100 + rng_seed)
    drv.reset()
    for _ in range(2):
        drv.step(rng.uniform(-1, 1, (N, drv.D)).astype(np.float32))
    drv.load_state(place(ora, drv.read_state(), rows, None if key is None else (key, family, N)))
    state = drv.read_state()
    a = rng.uniform(-1, 1, (N, drv.D)).astype(np.float32)
    drv.step(a)
    got = drv.outputs()
    # the oracle's own step from the shared state: switch mask, contact forces, what the family claims
    ora.load_state(state)
    ora.phys.margins = {}
    ora.step(a)
    mask = switch_mask(ora.phys.margins)
    by = {k: int((np.asarray(v) < SWITCH_EPS[k]).sum()) for k, v in ora.phys.margins.items()}
    ora.phys.margins = None
    want_cf = ora.contact_force.copy()
    peak = np.linalg.norm(ora.force_hist, axis=-1).max(axis=1)
    rep = dict(family=family, n=N, masked=int(mask.sum()), masked_by_margin=by)
    assert mask.mean() <= MAX_MASK, f"{family}: {int(mask.sum())} of {N} envs sit on a switch (> 1/8): {by}; envs {np.nonzero(mask)[0]}"
    if "c" in checks:
        rep["claims"] = check_claims(family, ora, state, rows, peak)
    if "a" in checks:
        try:
            tf = teacher_forced_check(ora, state, a, got, n_twins=n_twins, max_mask=MAX_MASK)
            assert_close("cforce", np.asarray(got["contact_force"])[~mask], want_cf[~mask], *CFORCE_BANDS)
        except AssertionError as e:
            raise AssertionError(f"check (a) {family}: {e}") from None
        rep["a"] = {f: tf[f]["max_err"] for f in ("root_state", "joint_vel", "obs_critic")}
        rep["cforce_max_err"] = float(np.abs(np.asarray(got["contact_force"], dtype=np.float64)[~mask] - want_cf[~mask]).max())
        rep["cforce_max"] = float(np.abs(want_cf).max())
    if "b" in checks:
        rep["b"] = check_lookup(ora, got, family)
    return rep


def profile_line(task, shape, rep):
    b = rep["b"]
    return (f"{task.split('-')[-2]:6s} {shape:10s} {rep['family']:9s} kernel {b['ratio']:7.3f}  fp32 restatement {b['ratio_fp32']:6.3f}  rays {b['rays']:6d}  "
            f"clipped -{b['clipped_lo']}/+{b['clipped_hi']}  masked {rep['masked']}/{rep['n']}" + (f"  base_height {b['base_height_ratio']:.3f}" if "base_height_ratio" in b else ""))


# ------------------------------------------------------------------------------------------------ check (d): defective samplers
class DefectiveSampler(TerrainSampler):
    """TerrainSampler with one defect a kernel's lookup could have.  Reads past the array's end are emulated on a copy padded with
    garbage (the kernel would read the next row, or memory that is not the heightfield's)."""

    DEFECTS = ("swap_index", "swap_normal", "cell_plus_one", "clamp_nx_1", "fraction_unclamped", "dzdy_sign")

    def __init__(self, tdesc, heights, defect):
        super().__init__(tdesc, heights)
        assert defect in self.DEFECTS
        self.defect = defect
        self.hp = np.full((tdesc.nx + 2, tdesc.ny + 2), 0.7)
        self.hp[: tdesc.nx, : tdesc.ny] = self.h

    def sample(self, x, y):
        t, d = self.t, self.defect
        gx, gy = (x - t.x0) / t.hscale, (y - t.y0) / t.hscale
        last = 1 if d == "clamp_nx_1" else 2
        ix = np.clip(np.floor(gx), 0, t.nx - last).astype(np.int64)
        iy = np.clip(np.floor(gy), 0, t.ny - last).astype(np.int64)
        fx, fy = gx - ix, gy - iy
        if d != "fraction_unclamped":
            fx, fy = np.clip(fx, 0.0, 1.0), np.clip(fy, 0.0, 1.0)
        if d == "cell_plus_one":
            ix = ix + 1
        if d == "swap_index":  # (ix, iy) for (iy, ix): the array read as [ny, nx]
            flat = self.h.reshape(-1)
            at = lambda a, b: flat[(b * t.nx + a) % flat.size]
        else:
            at = lambda a, b: self.hp[a, b]
        h00, h10, h01, h11 = at(ix, iy), at(ix + 1, iy), at(ix, iy + 1), at(ix + 1, iy + 1)
        hx0, hx1 = h00 + fx * (h10 - h00), h01 + fx * (h11 - h01)
        z = hx0 + fy * (hx1 - hx0)
        dzdx = ((1 - fy) * (h10 - h00) + fy * (h11 - h01)) / t.hscale
        dzdy = ((1 - fx) * (h01 - h00) + fx * (h11 - h10)) / t.hscale
        if d == "dzdy_sign":
            dzdy = -dzdy
        if d == "swap_normal":
            dzdx, dzdy = dzdy, dzdx
        inv = 1.0 / np.sqrt(dzdx * dzdx + dzdy * dzdy + 1.0)
        return z, np.stack([-dzdx * inv, -dzdy * inv, inv], -1)
