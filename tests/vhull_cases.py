"""Shared by tests/test_vhull.py (the CPU lane emulator) and tests/test_vhull_gpu.py (the C ABI on the GPU): the cases of
``enerf_vhull_bounds`` and its arbiter, a float64 numpy restatement of the model in include/enerf_hip.h.

The arbiter and the kernel evaluate the same double expressions in another order (the kernel's compiler may fuse a multiply-add), so a
voxel whose projection falls within rounding of a pixel boundary can go either way.  A voxel-view pair is UNDECIDED when the float64
``u + 0.5`` or ``v + 0.5`` lies within 1e-6 of an integer, or ``|c.z| < 1e-9``; occupancy is compared voxel by voxel wherever no pair
of the voxel is undecided, every face of ``bounds`` and every count must lie between the arbiter's value with all undecided voxels
carved and with all of them kept, and a case with more than 0.1 % undecided voxels fails outright.  The cameras' poses and principal
points are chosen off every 0.5 lattice of the grids, and the arbiter alone finds NO undecided voxel in any case below (UNDECIDED
records the counts, checked on every run), so every comparison here is in fact exact.  The one larger grid of the GPU file
(130 x 64 x 72, all-ones masks) has 10 undecided voxels of 599,040, 0.0017 %."""
import numpy as np
import torch

UNDECIDED_CAP = 1e-3
EPS_PIX, EPS_Z = 1e-6, 1e-9

# undecided voxels per case as the arbiter counts them on the CPU (case name -> count); `check` asserts them
UNDECIDED = {
    "ellipsoid": 0, "grid_3x5x2": 0, "grid_70x3x3": 0, "grid_1x1x1": 0, "grid_70x5x9_two_cus": 0,
    "layers_mm0_mv1": 0, "layers_mm0_mv2": 0, "layers_mm0_mv4": 0, "layers_mm1_mv1": 0, "layers_mm1_mv2": 0, "layers_mm1_mv4": 0,
    "abstention": 0, "guard": 0, "zero_masks": 0, "small_box": 0, "pad": 0, "replay_a": 0, "replay_b": 0,
}

# base_utils.get_bound_corners: row c of the eight corners takes x, y, z from bounds[CORNER_PATTERN[c][axis]]
CORNER_PATTERN = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]])

H, W = 48, 64
SCENE = np.array([[-1.3, -0.7, -0.35], [1.1, 0.9, 1.45]], np.float32)      # non-cubic, off-centre
CENTRE = np.array([-0.07, 0.13, 0.52])
RADII = np.array([0.62, 0.38, 0.71])
# the largest shrink of the ellipsoid about its centre for which every voxel centre inside it is occupied IN THE ARBITER (20x12x28 grid,
# min_views = V = 4, max_miss = 0) is 0.9433 (found on the CPU: the smallest |(p - centre) / radii| over the arbiter's empty voxels is
# 0.94336, a voxel whose nearest pixel centre just misses the silhouette); the tests ask for 0.943
ELLIPSOID_SHRINK = 0.943
# in the two-layer case every voxel centre inside the REAR ellipsoid shrunk by this is occupied at max_miss = 1 (the arbiter: 112 of 112
# such voxels, also at 0.95: 131 of 131) and most are lost at max_miss = 0 (22 of 112): camera 0 sees the front layer there
REAR_SHRINK = 0.9


# -- cameras -----------------------------------------------------------------------------------------
def look_at(pos, target, up=(0.0, 0.0, 1.0)):
    """World -> camera (4,4) float64 of a camera at ``pos`` looking at ``target``: x right, y down, z forward."""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    f = target - pos
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    E = np.eye(4)
    E[:3, :3] = np.stack([r, d, f])
    E[:3, 3] = -E[:3, :3] @ pos
    return E


def ring(V=4, radius=3.1, tilt=0.31, focal=58.7, h=H, w=W, target=CENTRE, phase=0.137):
    """V cameras on a ring tilted by ``tilt`` rad about x, irrational-looking angles and principal points: nothing on a 0.5 lattice."""
    exts, ixts = [], []
    ct, st = np.cos(tilt), np.sin(tilt)
    for v in range(V):
        a = phase + 2 * np.pi * v / V + 0.0173 * v * v
        p = np.array([np.cos(a), np.sin(a), 0.283 + 0.061 * v]) * radius
        p = np.array([p[0], ct * p[1] - st * p[2], st * p[1] + ct * p[2]]) + np.asarray(target)
        exts.append(look_at(p, np.asarray(target) + np.array([0.013 * v, -0.021, 0.017])))
        ixts.append(np.array([[focal + 0.37 * v, 0.0, w / 2 + 0.2371 - 0.113 * v], [0.0, focal + 1.13 - 0.29 * v, h / 2 - 0.3113 + 0.071 * v],
                              [0.0, 0.0, 1.0]]))
    return np.stack(exts).astype(np.float32), np.stack(ixts).astype(np.float32)


# -- masks, rasterised in float64 from analytic ellipsoids ---------------------------------------------
def raster(exts, ixts, objects, h=H, w=W):
    """(V,h,w) uint8: the label (1-based position in ``objects`` = [(centre, radii)]) of the nearest ellipsoid the ray through each
    pixel CENTRE hits, 0 where it hits none."""
    V = exts.shape[0]
    out = np.zeros((V, h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    for v in range(V):
        E, K = exts[v].astype(np.float64), ixts[v].astype(np.float64)
        R, t = E[:3, :3], E[:3, 3]
        o = -R.T @ t
        d = np.stack([(xx - K[0, 2]) / K[0, 0], (yy - K[1, 2]) / K[1, 1], np.ones_like(xx)], -1) @ R      # rows: R^T d
        best = np.full((h, w), np.inf)
        for label, (c, r) in enumerate(objects, 1):
            oc, ds = (o - np.asarray(c)) / np.asarray(r), d / np.asarray(r)
            A, B, C = (ds * ds).sum(-1), 2 * (ds * oc).sum(-1), (oc * oc).sum() - 1.0
            disc = B * B - 4 * A * C
            s = np.where(disc >= 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), np.inf)
            hit = (disc >= 0) & (s > 0) & (s < best)
            out[v][hit] = label
            best = np.where(hit, s, best)
    return out


# -- the arbiter ----------------------------------------------------------------------------------------
def voxel_centres(scene, grid):
    lo, hi = scene[0].astype(np.float64), scene[1].astype(np.float64)
    ax = [lo[a] + (np.arange(grid[a], dtype=np.float64) + 0.5) * (hi[a] - lo[a]) / grid[a] for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], -1)                                       # (Gz,Gy,Gx,3)


def box_of(occ, scene, grid, pad):
    """bounds (2,3) float32, count, flags of one layer's occupied voxels ``occ`` (Gz,Gy,Gx) bool."""
    n = int(occ.sum())
    if n == 0:
        return scene.astype(np.float32).copy(), 0, 1
    lo, hi = scene[0].astype(np.float64), scene[1].astype(np.float64)
    b, f = np.zeros((2, 3), np.float32), 0
    for a in range(3):
        idx = np.nonzero(occ.any(axis=tuple(d for d in range(3) if d != 2 - a)))[0]
        imin, imax = int(idx[0]), int(idx[-1])
        cell = (hi[a] - lo[a]) / grid[a]
        b[0, a] = np.float32((lo[a] + imin * cell) - pad)
        b[1, a] = np.float32((lo[a] + (imax + 1) * cell) + pad)
        if imin == 0 or imax == grid[a] - 1:
            f |= 2
    return b, n, f


def arbiter(masks, exts, ixts, scene, grid, n_layers=1, labels=False, min_views=2, max_miss=0, pad=0.0):
    masks = np.asarray(masks)
    V, h, w = masks.shape
    P = voxel_centres(scene, grid)
    inside = np.zeros((n_layers,) + P.shape[:3], np.int64)
    votes = np.zeros(P.shape[:3], np.int64)
    undecided, voted = np.zeros(P.shape[:3], bool), []
    with np.errstate(all="ignore"):
        for v in range(V):
            E, K = exts[v].astype(np.float64), ixts[v].astype(np.float64).reshape(9)
            c = P @ E[:3, :3].T + E[:3, 3]
            cx, cy, cz = c[..., 0], c[..., 1], c[..., 2]
            front = cz > 0
            u, vv = K[0] * cx / cz + K[2], K[4] * cy / cz + K[5]
            fu, fv = np.floor(u + 0.5), np.floor(vv + 0.5)
            seen = front & (fu >= 0) & (fu < w) & (fv >= 0) & (fv < h)
            near = lambda x: np.abs(x - np.rint(x)) < EPS_PIX             # noqa: E731  (NaN and inf compare False)
            undecided |= (np.abs(cz) < EPS_Z) | (front & (near(u + 0.5) | near(vv + 0.5)))
            iu, iv = np.where(seen, fu, 0).astype(np.int64), np.where(seen, fv, 0).astype(np.int64)
            m = masks[v][iv, iu]
            votes += seen
            voted.append(float(seen.mean()))
            for l in range(n_layers):
                inside[l] += seen & ((m == l + 1) if labels else (m != 0))
    occ = (inside >= min_views) & ((votes[None] - inside) <= max_miss)       # (L,Gz,Gy,Gx)
    return dict(occ=occ, undecided=undecided, voted=voted, scene=np.asarray(scene, np.float32), grid=tuple(grid), pad=float(pad), L=n_layers)


def run(lib, dev, masks, exts, ixts, scene, grid, **kw):
    """The kernel's outputs as numpy: bounds, counts, flags, corners, occupancy."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    occ = torch.full(tuple(grid)[::-1], 0xEE, dtype=torch.uint8, device=dev)
    bounds, counts, flags, corners = lib.vhull_bounds(t(masks), t(exts), t(ixts), scene, grid=grid, occupancy=occ, **kw)
    return dict(bounds=bounds.cpu().numpy(), counts=counts.cpu().numpy(), flags=flags.cpu().numpy(), corners=corners.cpu().numpy(),
                occupancy=occ.cpu().numpy())


def compare(name, got, arb):
    """The rules of the module's docstring; returns the number of undecided voxels."""
    und = arb["undecided"]
    n_und = int(und.sum())
    print(f"{name}: {n_und} undecided of {und.size} voxels")
    assert n_und <= UNDECIDED_CAP * und.size, (name, n_und, und.size)
    assert n_und == UNDECIDED[name], (name, n_und)
    scene, grid, pad = arb["scene"], arb["grid"], arb["pad"]
    assert not (got["occupancy"] >> arb["L"]).any()
    for l in range(arb["L"]):
        occ = arb["occ"][l]
        mine = (got["occupancy"] >> l) & 1 != 0
        assert np.array_equal(mine[~und], occ[~und]), (name, l, int((mine != occ)[~und].sum()))
        (bc, nc, fc), (bk, nk, fk) = box_of(occ & ~und, scene, grid, pad), box_of(occ | und, scene, grid, pad)
        n, b, f = int(got["counts"][l]), got["bounds"][l], int(got["flags"][l])
        assert nc <= n <= nk and n == int(mine.sum()), (name, l, nc, n, nk)
        if nc == nk:                                                     # the undecided voxels (if any) change nothing: exact
            assert np.array_equal(b, bc) and f == fc, (name, l, b, bc, f, fc)
        elif n == 0:
            assert np.array_equal(b, scene) and f == 1
        else:                                                            # (an empty carved set constrains nothing from inside)
            assert np.all(bk[0] <= b[0]) and np.all(b[1] <= bk[1]), (name, l)
            assert nc == 0 or (np.all(b[0] <= bc[0]) and np.all(bc[1] <= b[1])), (name, l)
        want = np.stack([b[CORNER_PATTERN[:, a], a] for a in range(3)], -1)
        assert np.array_equal(got["corners"][l], want), (name, l)
    return n_und


def check(lib, dev, name, masks, exts, ixts, scene, grid, **kw):
    got = run(lib, dev, masks, exts, ixts, scene, grid, **kw)
    arb = arbiter(masks, exts, ixts, np.asarray(scene, np.float32), grid, **kw)
    compare(name, got, arb)
    return got, arb


# -- the cases ---------------------------------------------------------------------------------------------
def ellipsoid_case():
    exts, ixts = ring()
    return raster(exts, ixts, [(CENTRE, RADII)]), exts, ixts, SCENE, (20, 12, 28)


def ellipsoid_depth(scene, grid):
    """|(p - centre) / radii| of every voxel centre: < 1 inside the ellipsoid."""
    return np.linalg.norm((voxel_centres(np.asarray(scene, np.float32), grid) - CENTRE) / RADII, axis=-1)


# two labelled ellipsoids; from camera 0 (and only there) the front one covers part of the rear one
FRONT = (np.array([0.55, 0.05, 0.45]), np.array([0.30, 0.33, 0.42]))
REAR = (np.array([-0.35, 0.12, 0.50]), np.array([0.34, 0.30, 0.45]))


def layers_case():
    exts, ixts = ring(target=np.array([0.1, 0.08, 0.48]), phase=0.037)
    return raster(exts, ixts, [FRONT, REAR]), exts, ixts, SCENE, (22, 14, 18)


def abstention_case():
    """The ring's four cameras and four that mostly abstain: one INSIDE the scene box (voxels behind it), one looking away from the
    box, one whose ext holds NaN, one with fx = 0.  Their masks are all ones: where they do vote, they vote inside."""
    exts, ixts = ring()
    masks = raster(exts, ixts, [(CENTRE, RADII)])
    e2, k2 = ring(phase=0.731)
    e2[0] = look_at([0.31, 0.17, 0.61], [0.9, -0.55, 0.2]).astype(np.float32)                  # inside the box
    e2[1] = look_at([3.0, 2.0, 1.0], [6.0, 4.1, 1.7]).astype(np.float32)                      # the box is behind it
    e2[2, 1, 2] = np.nan
    k2[3, 0, 0] = 0.0
    return (np.concatenate([masks, np.ones_like(masks)]), np.concatenate([exts, e2]), np.concatenate([ixts, k2]), SCENE, (18, 10, 14))


def two_time_frames(V, h, w, exts, ixts):
    """Two time frames' masks for cameras (V of them, any rig): an ellipsoid that moves, as [(V,h,w) uint8] * 2."""
    return [raster(exts, ixts, [(c, r)], h, w) for c, r in ((np.array([0.0, 0.0, 0.0]), np.array([0.5, 0.4, 0.6])),
                                                            (np.array([0.25, -0.1, 0.1]), np.array([0.35, 0.5, 0.4])))]


# -- what both test files run: every function takes the library and the device -------------------------------
GRID_SHAPES = {"grid_3x5x2": (3, 5, 2), "grid_70x3x3": (70, 3, 3), "grid_1x1x1": (1, 1, 1)}


def case_ellipsoid(lib, dev):
    masks, exts, ixts, scene, grid = ellipsoid_case()
    got, arb = check(lib, dev, "ellipsoid", masks, exts, ixts, scene, grid, min_views=4, max_miss=0)
    inside = ellipsoid_depth(scene, grid) <= ELLIPSOID_SHRINK
    assert inside.sum() > 400 and bool(arb["occ"][0][inside].all())      # the arbiter itself satisfies it (and 0.944 would not)
    assert not arb["occ"][0][ellipsoid_depth(scene, grid) <= 0.944].all()
    assert bool(((got["occupancy"] & 1) != 0)[inside].all())
    assert int(got["flags"][0]) == 0 and 0 < int(got["counts"][0]) < inside.size // 4


def case_grid(lib, dev, name):
    masks, exts, ixts, scene, _ = ellipsoid_case()
    got, _ = check(lib, dev, name, masks, exts, ixts, scene, GRID_SHAPES[name], min_views=2, max_miss=0)
    return got


def case_layers(lib, dev):
    masks, exts, ixts, scene, grid = layers_case()
    V = masks.shape[0]
    assert set(np.unique(masks)) == {0, 1, 2}
    rear = np.linalg.norm((voxel_centres(np.asarray(scene, np.float32), grid) - REAR[0]) / REAR[1], axis=-1) < REAR_SHRINK
    got = {}
    for mm in (0, 1):
        for mv in (1, 2, V):
            got[mm, mv], _ = check(lib, dev, f"layers_mm{mm}_mv{mv}", masks, exts, ixts, scene, grid, n_layers=2, labels=True, min_views=mv,
                                   max_miss=mm)
    occ_rear = lambda g: ((g["occupancy"] >> 1) & 1 != 0)                  # noqa: E731
    lost, back = occ_rear(got[0, 2])[rear], occ_rear(got[1, 2])[rear]
    assert rear.sum() > 100 and 0 < lost.sum() < rear.sum() // 2 and bool(back.all())        # max_miss = 0 loses it, 1 recovers it
    assert int(got[1, V]["counts"][1]) < int(got[1, 2]["counts"][1])      # min_views = V leaves no view to miss


def case_abstention(lib, dev):
    masks, exts, ixts, scene, grid = abstention_case()
    got, arb = check(lib, dev, "abstention", masks, exts, ixts, scene, grid, min_views=2, max_miss=0)
    assert 0 < int(got["counts"][0]) < arb["undecided"].size
    share = arb["voted"]                                                  # the share of the voxels each view votes on
    assert all(s > 0.9 for s in share[:4]) and 0.0 < share[4] < 0.5 and share[5] == 0.0 and share[6] == 0.0 and 0.0 < share[7]


def case_guard(lib, dev):
    """All-zero masks in the middle of a buffer of ones: a read outside the masks would be a vote inside, and with min_views = 1 and
    max_miss = V one such vote occupies the voxel."""
    _, exts, ixts, scene, grid = abstention_case()
    V = exts.shape[0]
    buf = torch.ones((3 * V * H * W,), dtype=torch.uint8)
    buf[V * H * W:2 * V * H * W] = 0
    buf = buf.to(dev)
    masks = buf[V * H * W:2 * V * H * W].view(V, H, W)
    t = lambda a: torch.from_numpy(a).to(dev)                              # noqa: E731
    bounds, counts, flags, _ = lib.vhull_bounds(masks, t(exts), t(ixts), scene, grid=grid, min_views=1, max_miss=V)
    assert int(counts[0]) == 0 and int(flags[0]) == 1 and np.array_equal(bounds[0].cpu().numpy(), scene)
    got, _ = check(lib, dev, "guard", masks.cpu().numpy(), exts, ixts, scene, grid, min_views=1, max_miss=V)


def case_flags(lib, dev):
    masks, exts, ixts, scene, grid = ellipsoid_case()
    got, _ = check(lib, dev, "zero_masks", np.zeros_like(masks), exts, ixts, scene, grid, min_views=2, pad=0.25)
    assert int(got["flags"][0]) == 1 and int(got["counts"][0]) == 0 and np.array_equal(got["bounds"][0], scene)      # (no pad either)
    small = np.array([[-0.4, -0.2, 0.2], [0.25, 0.3, 0.9]], np.float32)   # inside the ellipsoid along every axis
    got, _ = check(lib, dev, "small_box", masks, exts, ixts, small, (9, 7, 11), min_views=4)
    assert int(got["flags"][0]) == 2 and np.array_equal(got["bounds"][0], small)
    pad = 0.0371
    plain, _ = check(lib, dev, "ellipsoid", masks, exts, ixts, scene, grid, min_views=4)
    got, arb = check(lib, dev, "pad", masks, exts, ixts, scene, grid, min_views=4, pad=pad)
    lo, hi = scene[0].astype(np.float64), scene[1].astype(np.float64)
    for a in range(3):                                                    # the float32 rounding of the double sum, restated
        idx = np.nonzero(arb["occ"][0].any(axis=tuple(d for d in range(3) if d != 2 - a)))[0]
        cell = (hi[a] - lo[a]) / grid[a]
        assert got["bounds"][0, 0, a] == np.float32(lo[a] + idx[0] * cell - pad) and got["bounds"][0, 0, a] < plain["bounds"][0, 0, a]
        assert got["bounds"][0, 1, a] == np.float32(lo[a] + (idx[-1] + 1) * cell + pad) and got["bounds"][0, 1, a] > plain["bounds"][0, 1, a]
    assert np.array_equal(got["counts"], plain["counts"]) and np.array_equal(got["occupancy"], plain["occupancy"])


def case_determinism(lib, dev):
    masks, exts, ixts, scene, grid = layers_case()
    a = run(lib, dev, masks, exts, ixts, scene, grid, n_layers=2, labels=True, min_views=2, max_miss=1)
    b = run(lib, dev, masks, exts, ixts, scene, grid, n_layers=2, labels=True, min_views=2, max_miss=1)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    # bool masks are viewed as uint8
    masks, exts, ixts, scene, grid = ellipsoid_case()
    t = lambda x: torch.from_numpy(x).to(dev)                              # noqa: E731
    u8 = lib.vhull_bounds(t(masks), t(exts), t(ixts), scene, grid=grid)
    bl = lib.vhull_bounds(t(masks != 0), t(exts), t(ixts), scene, grid=grid)
    assert all(torch.equal(p, q) for p, q in zip(u8, bl))


def case_corners(lib, dev):
    """``corners`` as the vertices of bounds_near_far and ``bounds`` as layer_boxes' input give what the same numbers give when they
    come from the host (here: the arbiter's box, uploaded)."""
    masks, exts, ixts, scene, grid = layers_case()
    kw = dict(n_layers=2, labels=True, min_views=2, max_miss=1)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)        # noqa: E731
    bounds, counts, flags, corners = lib.vhull_bounds(t(masks), t(exts), t(ixts), scene, grid=grid, **kw)
    arb = arbiter(masks, exts, ixts, scene, grid, **kw)
    assert not arb["undecided"].any()
    host = np.stack([box_of(arb["occ"][l], scene, grid, 0.0)[0] for l in range(2)])
    host_corners = np.stack([host[:, CORNER_PATTERN[:, a], a] for a in range(3)], -1)          # (L,8,3)
    assert np.array_equal(corners.cpu().numpy(), host_corners)
    tar_ext, tar_ixt = t(exts[1:2]), t(ixts[1:2])
    for l in range(2):
        assert torch.equal(lib.bounds_near_far(corners[l], tar_ext, 0.05), lib.bounds_near_far(t(host_corners[l]), tar_ext, 0.05))
    sizes = [(32, 32), (32, 32)]
    mine, theirs = lib.layer_boxes(bounds, tar_ext, tar_ixt, H, W, sizes, 0.05), lib.layer_boxes(t(host), tar_ext, tar_ixt, H, W, sizes, 0.05)
    assert all(torch.equal(p, q) for p, q in zip(mine, theirs)) and int(mine[2].max()) & 4 == 0


def case_refusals(lib, dev):
    from enerf_amd.lib import EnerfError, VhullArgs
    import ctypes as C
    masks, exts, ixts, scene, grid = ellipsoid_case()
    t = lambda x: torch.from_numpy(x).to(dev)                              # noqa: E731
    m, e, k = t(masks), t(exts), t(ixts)
    out = (torch.full((1, 2, 3), 7.0, device=dev), torch.full((1,), 7, dtype=torch.int32, device=dev),
           torch.full((1,), 7, dtype=torch.int32, device=dev), torch.full((1, 8, 3), 7.0, device=dev))
    occ = torch.full(grid[::-1], 7, dtype=torch.uint8, device=dev)
    ws = torch.full((64,), 7, dtype=torch.int32, device=dev)
    call, err, stream = lib.dll.enerf_vhull_bounds, lib.dll.enerf_last_error, lib.stream_of(m)

    def args(**kw):
        a = VhullArgs(masks=m.data_ptr(), exts=e.data_ptr(), ixts=k.data_ptr(), V=4, H=H, W=W, n_layers=1, labels=0, min_views=2, max_miss=0,
                      pad=0.0, bounds=out[0].data_ptr(), counts=out[1].data_ptr(), flags=out[2].data_ptr(), corners=out[3].data_ptr(),
                      occupancy=occ.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=256)
        for i in range(6):
            a.scene_bounds[i // 3][i % 3] = float(scene[i // 3][i % 3])
        for i in range(3):
            a.grid[i] = grid[i]
        for key, v in kw.items():
            if key == "grid":
                for i in range(3):
                    a.grid[i] = v[i]
            elif key == "scene":
                for i in range(6):
                    a.scene_bounds[i // 3][i % 3] = v[i // 3][i % 3]
            else:
                setattr(a, key, v)
        return a

    def refused(text, **kw):
        assert call(C.byref(args(**kw)), stream) == -1 and text in err(), (text, kw, err())

    assert call(None, stream) == -1 and b"null args" in err()
    for name in ("masks", "exts", "ixts", "bounds", "counts", "flags", "corners", "workspace"):
        refused(b"null " + name.encode(), **{name: None})
    for g in ((0, 4, 4), (4, 257, 4), (4, 4, -1)):
        refused(b"grid", grid=g)
    for L in (0, 5, -1):
        refused(b"foreground layers", n_layers=L, labels=1)
    refused(b"need labels", n_layers=2, labels=0)
    refused(b"min_views", min_views=0)
    refused(b"max_miss", max_miss=-1)
    for pad in (-0.5, float("nan"), float("inf")):
        refused(b"pad", pad=pad)
    for sc in (((0, 0, 0), (1, 0, 1)), ((0, 0, 2), (1, 1, 1)), ((0, float("nan"), 0), (1, 1, 1)), ((0, 0, 0), (1, float("inf"), 1))):
        refused(b"scene_bounds", scene=sc)
    refused(b"bytes", workspace_bytes=16)
    refused(b"V=", V=0)
    refused(b"V=", V=65)
    refused(b"mask extent", H=0)
    assert lib.dll.enerf_vhull_workspace_bytes(None) == 0 and b"null args" in err()
    assert lib.dll.enerf_vhull_workspace_bytes(C.byref(args(n_layers=9))) == 0 and b"foreground layers" in err()
    assert lib.dll.enerf_vhull_workspace_bytes(C.byref(args(n_layers=4))) == 4 * 32
    if dev != "cpu" and torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    for x in out + (occ, ws):                                             # nothing was enqueued
        assert bool((x == 7).all())
    assert call(C.byref(args()), stream) == 0
    assert int(out[1][0]) > 0 and int(out[2][0]) == 0 and bool((occ <= 1).all())
    with pytest_raises(EnerfError, "uint8 / bool"):
        lib.vhull_bounds(m.float(), e, k, scene, grid=grid)
    with pytest_raises(EnerfError, r"exts must be .*\(4, 4, 4\)"):
        lib.vhull_bounds(m, e[:3], k, scene, grid=grid)
    with pytest_raises(EnerfError, "out bounds"):
        lib.vhull_bounds(m, e, k, scene, grid=grid, out=(out[0][0], out[1], out[2], out[3]))
    with pytest_raises(EnerfError, "occupancy must be"):
        lib.vhull_bounds(m, e, k, scene, grid=grid, occupancy=occ.view(-1))
    with pytest_raises(EnerfError, "need labels"):
        lib.vhull_bounds(m, e, k, scene, grid=grid, n_layers=2)


def pytest_raises(exc, match):
    import pytest
    return pytest.raises(exc, match=match)


# -- the sequence player ------------------------------------------------------------------------------------
PLAYER_SCENE = ((-160.0, -130.0, 480.0), (170.0, 140.0, 860.0))          # around the synthetic rig's point of regard
PLAYER_HULL = dict(grid=(12, 10, 8), min_views=3, max_miss=2, pad=1.5)


def case_player(lib, dev, net, cfg, raw):
    """Two time frames with different masks: after each flip the player's bounds, counts, flags and corners are bit for bit the direct
    call on that frame's masks (with raw=: on the ingest's mask_out); renders go on as without a hull."""
    import ingest_raw_cases as R
    from enerf_amd.sequence import HullSpec, SequencePlayer
    from sequence_cases import CAMERAS, assert_same, time_frames
    Hp, Wp, V, dilate = 32, 64, 5, 5
    frames, exts, ixts, tar = time_frames(cfg, Hp, Wp, V, seeds=(3, 4))
    exts, tar = exts.to(dev), {k: v.to(dev) for k, v in tar.items()}
    rig = None
    if raw:
        rig = R.wired_rig(lib, dev, ixts, 2 * Hp, 2 * Wp, 0.5)
        frames = R.raw_time_frames(V, 2 * Hp, 2 * Wp, (3, 4))
    cam_ixts = rig.ixts if raw else ixts.to(dev)
    spec = HullSpec(PLAYER_SCENE, **PLAYER_HULL)
    player = SequencePlayer(net, exts, cam_ixts, Hp, Wp, slots=2, dilate=dilate, raw=rig, hull=spec)
    plain = SequencePlayer(net, exts, cam_ixts, Hp, Wp, slots=2, dilate=dilate, raw=rig)
    assert plain.hull is None and all(s.hull is None for s in plain.slots)
    idx = torch.tensor(CAMERAS[0], dtype=torch.int32, device=dev)
    seen = []
    for t, (u8, mask) in enumerate(frames):
        player.submit(u8, mask)
        player.flip()
        mine = [x.clone() for x in (player.bounds, player.hull_counts, player.hull_flags, player.corners)]
        out = {k: v.clone() for k, v in player.render(idx, tar).items()}
        if raw:
            final = torch.empty((V, Hp, Wp), dtype=torch.uint8, device=dev)
            rig(u8.to(dev), mask.to(dev), dilate, mask_out=final)
        else:
            final = mask.to(dev)
        direct = lib.vhull_bounds(final, exts, cam_ixts, PLAYER_SCENE, **PLAYER_HULL)
        for p, q in zip(mine, direct):
            assert torch.equal(p, q), t
        assert int(direct[1][0]) > 0 and int(direct[2][0]) & 1 == 0
        seen.append(mine[0])
        if t == 0:                                                        # hull=None: submit / render as ever, and the same bits
            plain.submit(u8, mask)
            plain.flip()
            assert_same(plain.render(idx, tar), out)
            with pytest_raises(RuntimeError, "without hull="):
                plain.bounds
    assert not torch.equal(seen[0], seen[1])
    with pytest_raises(ValueError, "pass masks"):
        player.submit(frames[0][0])
