"""Float64 restatement of openmpl_amd/rpsm.py (csrc/rpsm.hip) and the deterministic cases of its tests (TEST INFRASTRUCTURE ONLY).

numpy float64 on the float32 inputs the kernels read.  It is pinned by tests/golden/rpsm.npz, which the reference's own compute_grid,
compute_unary_term, compute_pairwise_constrain, infer and rpsm produced (tests/golden/make_golden_rpsm.py).

A case: a roughly human pose in millimetres, cameras on a ring about 4.5 m out looking at it, per view and joint a Gaussian at the
joint's cell plus a small positive random floor, limb lengths taken from the pose, the root centre a few centimetres off.  Every
case is built until two conditions hold on its own restatement, so that bins compare exactly with no case left out:
 (a) every | | d - limb | - tolerance | over the pairs of the first grid is at least MARGIN_A = 1e-6 (d = sqrt(m) * step over the
     integers m = dix^2 + diy^2 + diz^2; the rounded coordinates move d by less than 1e-9);
 (b) on the chosen path (the root's argmax and every back-pointer followed, in every round) the gap between the maximum and the
     runner-up is exactly 0 with both values 0, or at least MARGIN_B = 1e-9 of the maximum: an fp64 reordering of at most 32 views x
     4 products x 64 joints stays below about 1e-12 relative.
A case that violates either gets another seed, never an exclusion.
"""
import functools
import os

import numpy as np

from openmpl_amd import detrng

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN_A, MARGIN_B = 1e-6, 1e-9
Z_MIN = 1e-9
BODY = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)          # lib/multiviews/body.py as parents
# root rhip rkne rank lhip lkne lank belly neck nose head lsho lelb lwri rsho relb rwri, millimetres about the root, z up
TEMPLATE = np.array([[0, 0, 0], [-130, 0, 0], [-140, 20, -440], [-150, 0, -880], [130, 0, 0], [140, 30, -440], [150, 10, -880], [0, -10, 250],
                     [0, 0, 500], [0, 70, 600], [0, 20, 700], [170, 0, 470], [260, 40, 220], [300, 120, 0], [-170, 0, 470], [-280, 60, 230],
                     [-330, 160, 40]], np.float64)
TREES = {"body": (BODY, tuple(range(17))), "single": ((-1,), (0,)), "chain": ((-1, 0, 1), (0, 7, 8)),
         "star": ((-1, 0, 0, 0, 0), (0, 1, 4, 7, 12))}
IMAGE = (256.0, 256.0)


# ------------------------------------------------------------------------------------------------------------ restatement
def grid(size, c, n):
    l = np.linspace(-size / 2, size / 2, n)
    gx, gy, gz = np.meshgrid(l + c[0], l + c[1], l + c[2])                    # the default xy indexing: y slowest, z fastest
    return np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1)


def crop_cells(px, center, scale_x, image_size, W, H):
    """image pixels (N,2) -> heatmap cells, the closed form of get_affine_transform(center, scale, 0, image_size) and * (W,H) / size"""
    iw, ih = float(image_size[0]), float(image_size[1])
    k = iw / (200.0 * float(scale_x))
    ux = ((px[:, 0] - float(center[0])) * k + iw * 0.5) * W / iw
    uy = ((px[:, 1] - float(center[1])) * k + ih * 0.5) * H / ih
    return np.stack([ux, uy], axis=1)


def project(X, cam, dist=None):
    """(N,3) world -> (N,2) pixels and z_cam; cam: a (16,) row of pack_cameras; dist: k1 k2 k3 p1 p2 or None"""
    f, c, R, t = cam[0:2], cam[2:4], cam[4:13].reshape(3, 3), cam[13:16]
    xc = (X - t) @ R.T
    z = xc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        y = xc[:, :2] / z[:, None]
    k1, k2, k3, p1, p2 = (0.0,) * 5 if dist is None else [float(d) for d in dist]
    r2 = (y ** 2).sum(1)
    g = 1.0 + (k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) + (2.0 * p1 * y[:, 1] + 2.0 * p2 * y[:, 0])
    y = y * g[:, None] + np.outer(r2, [p2, p1])
    return f * y + c, z


def bilinear(hmap, u):
    """hmap (H,W), u (N,2) cells -> (N,), 0 outside [0,W-1] x [0,H-1]"""
    H, W = hmap.shape
    hmap = hmap.astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = (u[:, 0] >= 0) & (u[:, 0] <= W - 1) & (u[:, 1] >= 0) & (u[:, 1] <= H - 1)
    ux, uy = np.where(inside, u[:, 0], 0.0), np.where(inside, u[:, 1], 0.0)
    x0, y0 = np.minimum(ux.astype(np.int64), W - 2), np.minimum(uy.astype(np.int64), H - 2)
    tx, ty = ux - x0, uy - y0
    val = ((hmap[y0, x0] * ((1 - tx) * (1 - ty)) + hmap[y0 + 1, x0] * ((1 - tx) * ty)) + hmap[y0, x0 + 1] * (tx * (1 - ty))) \
        + hmap[y0 + 1, x0 + 1] * (tx * ty)
    return np.where(inside, val, 0.0)


def unary(hm, grids, center, scale, cams, image_size, dist=None):
    """hm (V,J,H,W); grids: one shared (N,3) or J of them -> (J,N)"""
    V, J, H, W = hm.shape
    out = np.zeros((J, grids[0].shape[0]))
    for j in range(J):
        g = grids[0] if len(grids) == 1 else grids[j]
        for v in range(V):
            px, z = project(g, cams[v], None if dist is None else dist[v])
            s = bilinear(hm[v, j], crop_cells(px, center[v], scale[v][0], image_size, W, H))
            out[j] = out[j] + np.where(z <= Z_MIN, 0.0, s)
    return out


def children_of(parents):
    return [[c for c, q in enumerate(parents) if q == j] for j in range(len(parents))]


def depths(parents):
    d = []
    for j in range(len(parents)):
        k, n = j, 0
        while parents[k] != -1:
            k, n = parents[k], n + 1
        d.append(n)
    return d


def candidates(gp, gc, limb, tol, ec, rows=None):
    """the candidate matrix of an edge (all parent bins, or `rows` of them): the child's energy where allowed, else 0.0"""
    gp = gp if rows is None else gp[rows]
    d = np.sqrt(((gp[:, None, :] - gc[None, :, :]) ** 2).sum(-1))
    return np.where(np.abs(d - limb) <= tol, ec[None, :], 0.0)


def first_argmax(val):
    """np.argmax along the last axis (NaN counts as the maximum, the first one wins) and the value there"""
    i = np.argmax(val, axis=-1)
    return i, np.take_along_axis(val, i[..., None], -1)[..., 0]


def gap(row):
    """relative gap between the maximum and the runner-up of a candidate row, 0 only when both are 0"""
    if row.size < 2 or np.isnan(row).any():
        return np.inf
    top = np.sort(row)[-2:]
    if top[1] == top[0]:
        return np.inf if top[1] == 0.0 else 0.0
    return (top[1] - top[0]) / abs(top[1])


def infer(U, grids, parents, limb, tol):
    """U (J,N), grids (one shared or J) -> bins (J,), the root's maximum, the smallest gap on the chosen path"""
    J = len(parents)
    kids, dep = children_of(parents), depths(parents)
    root = parents.index(-1)
    g = lambda j: grids[0] if len(grids) == 1 else grids[j]
    E, back = U.copy(), {}
    chunk = 512
    for node in sorted(range(J), key=lambda j: -dep[j]):
        for c in kids[node]:
            mv, mi = np.empty(E.shape[1]), np.empty(E.shape[1], np.int64)
            for s in range(0, E.shape[1], chunk):
                rows = np.arange(s, min(s + chunk, E.shape[1]))
                mi[rows], mv[rows] = first_argmax(candidates(g(node), g(c), limb[c], tol, E[c], rows))
            E[node] = E[node] * mv
            back[c] = mi
    bins = np.zeros(J, np.int64)
    bins[root], energy = first_argmax(E[root])
    margin = gap(E[root])
    for c in sorted(range(J), key=lambda j: dep[j]):
        if c != root:
            bins[c] = back[c][bins[parents[c]]]
            margin = min(margin, gap(candidates(g(parents[c]), g(c), limb[c], tol, E[c], np.array([bins[parents[c]]]))[0]))
    return bins, float(energy), margin


def solve_one(hm, center, scale, cams, image_size, root_center, limb, parents, first_nbins=16, recur_nbins=2, recur_depth=10,
              grid_size=2000.0, tolerance=150.0, dist=None):
    """one pose: hm (V,J,H,W) -> dict(poses (J,3) float64, bins (1 + depth, J), energy, margin, first (J,3) the first round's points)"""
    parents = list(parents)
    J = len(parents)
    limb = np.asarray(limb, np.float64)
    hm = np.asarray(hm)
    g0 = grid(grid_size, np.asarray(root_center, np.float64), first_nbins)
    b, energy, margin = infer(unary(hm, [g0], center, scale, cams, image_size, dist), [g0], parents, limb, tolerance)
    bins, pose = [b], g0[b]
    first = pose.copy()
    cur = grid_size / first_nbins
    for _ in range(recur_depth):
        grids = [grid(cur, pose[j], recur_nbins) for j in range(J)]
        b, _, m = infer(unary(hm, grids, center, scale, cams, image_size, dist), grids, parents, limb, tolerance)
        margin = min(margin, m)
        bins.append(b)
        pose = np.stack([grids[j][b[j]] for j in range(J)])
        cur = cur / recur_nbins
    return dict(poses=pose, bins=np.stack(bins).astype(np.int32), energy=energy, margin=margin, first=first)


def solve(inp):
    """a whole case -> poses (B,J,3) float64, bins (B, 1 + depth, J) int32, energy (B,), margin (the smallest of the batch)"""
    B = inp["hm"].shape[0]
    limb = inp["limb"]
    outs = [solve_one(inp["hm"][b], inp["center"][b], inp["scale"][b], inp["cams"], inp["image_size"], inp["root_center"][b],
                      limb if limb.ndim == 1 else limb[b], inp["parents"], dist=inp["dist"], **inp["kw"]) for b in range(B)]
    return dict(poses=np.stack([o["poses"] for o in outs]), bins=np.stack([o["bins"] for o in outs]),
                energy=np.array([o["energy"] for o in outs]), margin=min(o["margin"] for o in outs),
                first=np.stack([o["first"] for o in outs]))


def boundary_distance(inp):
    """condition (a): the smallest | | sqrt(m) step - limb | - tolerance | over the offsets of the first grid and the limbs read"""
    n, size, tol = inp["kw"]["first_nbins"], inp["kw"]["grid_size"], inp["kw"]["tolerance"]
    d = np.sqrt(np.arange(3 * (n - 1) ** 2 + 1, dtype=np.float64)) * (size / (n - 1))
    limbs = np.asarray(inp["limb"], np.float64).reshape(-1, len(inp["parents"]))[:, [j for j, q in enumerate(inp["parents"]) if q != -1]]
    if limbs.size == 0:
        return np.inf
    return float(np.abs(np.abs(d[:, None] - limbs.reshape(1, -1)) - tol).min())


# ------------------------------------------------------------------------------------------------------------------ cases
def look_at(centre, aim):
    z = (aim - centre) / np.linalg.norm(aim - centre)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def render(cells, H, W, sigma, floor):
    """Gaussians of height 1 at `cells` (..., 2) plus the floor (..., H, W) -> float32 maps"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    g = np.exp(-((xx - cells[..., 0, None, None]) ** 2 + (yy - cells[..., 1, None, None]) ** 2) / (2.0 * sigma * sigma))
    return (g + floor).astype(np.float32)


def inputs(B=1, V=4, tree="body", H=64, W=64, seed=0, first_nbins=8, recur_nbins=2, recur_depth=10, grid_size=2000.0, tolerance=150.0,
           distortion=False, per_sample_limbs=False, off=40.0, nan=False, sigma=None):
    """the arrays of one case (no restatement): hm (B,V,J,H,W) float32, center / scale (B,V,2) float32, cams (V,16) float64, dist (V,5)
    float64 or None, root_center (B,3) float32, limb (J,) or (B,J) float32, parents, truth (B,J,3) float64, kw.  sigma: of the Gaussians,
    in cells (default 2 at 64 cells; a coarse first grid needs wider ones to see a joint that lies between its points)"""
    parents, pick = TREES[tree]
    J = len(parents)
    tag = "rpsm.%s.%d.%d.%dx%d" % (tree, B, V, H, W)
    u = lambda name, shape, lo, hi: detrng.uniform(seed, tag + "." + name, shape, lo, hi).astype(np.float64)
    base = TEMPLATE[list(pick)]
    truth = np.empty((B, J, 3))
    for b in range(B):
        a = u("turn%d" % b, (1,), 0.0, 2 * np.pi)[0]
        Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        body = (base + u("jitter%d" % b, (J, 3), -30.0, 30.0)) * (1.0 + 0.08 * b if per_sample_limbs else 1.0)
        truth[b] = body @ Rz.T + np.array([0.0, 0.0, 950.0]) + u("place%d" % b, (3,), -200.0, 200.0)
    az = 2 * np.pi * (np.arange(V) + u("az", (V,), 0.0, 0.4)) / max(V, 3)
    rad, hgt = u("rad", (V,), 4200.0, 4800.0), u("hgt", (V,), 1000.0, 2500.0)
    cams = []
    for v in range(V):
        c = np.array([rad[v] * np.cos(az[v]), rad[v] * np.sin(az[v]), hgt[v]])
        cams.append(np.concatenate([[1100.0 + 23.0 * v, 1090.0 - 17.0 * v, 500.0 + 9.0 * v, 500.0 - 6.0 * v],
                                    look_at(c, np.array([0.0, 0.0, 1000.0])).reshape(-1), c]))
    cams = np.stack(cams)
    dist = None
    if distortion:
        dist = np.stack([np.array([-0.2, 0.05, 0.01, 0.001, -0.002]) * (1.0 + 0.1 * v) for v in range(V)])
    center, scale = np.empty((B, V, 2), np.float32), np.empty((B, V, 2), np.float32)
    cells = np.empty((B, V, J, 2))
    for b in range(B):
        for v in range(V):
            px, _ = project(truth[b], cams[v], None if dist is None else dist[v])
            root_px, _ = project(truth[b][:1] + np.array([[0.0, 0.0, 50.0]]), cams[v], None if dist is None else dist[v])
            # quarter pixels and sixteenths: the reference rounds the anchor points of its affine fit to float32, which is exact here
            center[b, v] = (np.round((root_px[0] + u("box%d.%d" % (b, v), (2,), -15.0, 15.0)) * 4.0) / 4.0).astype(np.float32)
            scale[b, v] = np.float32(2.75 + 0.125 * v + 0.0625 * b)
            cells[b, v] = crop_cells(px, center[b, v], scale[b, v][0], IMAGE, W, H)
    floor = u("floor", (B, V, J, H, W), 0.001, 0.01)
    hm = render(cells, H, W, sigma if sigma else (2.0 * W / 64.0 if W >= 32 else 0.8), floor)
    if nan:
        hm[0, V - 1, J - 1, H // 2, W // 2] = np.nan
    limb = np.zeros((B, J))
    for j, q in enumerate(parents):
        if q != -1:
            limb[:, j] = np.linalg.norm(truth[:, j] - truth[:, q], axis=-1)
    limb = limb.astype(np.float32) if per_sample_limbs else limb[0].astype(np.float32)
    root_center = (truth[:, parents.index(-1)] + u("off", (B, 3), -off, off)).astype(np.float32)
    kw = dict(first_nbins=first_nbins, recur_nbins=recur_nbins, recur_depth=recur_depth, grid_size=float(grid_size), tolerance=float(tolerance))
    return dict(hm=hm, center=center, scale=scale, cams=cams, dist=dist, root_center=root_center, limb=limb, parents=list(parents),
                truth=truth, image_size=IMAGE, kw=kw)


def conditions(inp, ref):
    """(a) and (b) of the module docstring"""
    return boundary_distance(inp) >= MARGIN_A and ref["margin"] >= MARGIN_B


# name -> keyword arguments of inputs().  The shapes the GPU tests cover; every one is the smallest at which a path can go wrong.
CASES = {
    "n2": dict(tree="chain", first_nbins=2, grid_size=900.0, tolerance=700.0, recur_depth=3, sigma=6.0),      # 8 bins, below a wave
    "n3": dict(tree="star", first_nbins=3, grid_size=900.0, tolerance=350.0, recur_depth=3, sigma=6.0),       # 27 bins; the multi-child product
    "n5": dict(tree="star", first_nbins=5, grid_size=1200.0, tolerance=160.0, recur_depth=3, V=2, sigma=5.0),  # 125 bins, a ragged wave
    "n8": dict(first_nbins=8),                                                                       # 512 bins, the default tree
    "n11": dict(first_nbins=11, recur_depth=1, V=2),                                                 # 1331 bins, ragged against 256
    "single": dict(tree="single", first_nbins=5, grid_size=600.0, V=1, recur_depth=3, sigma=4.0),               # no edge, one view
    "chain_r3": dict(tree="chain", first_nbins=8, recur_nbins=3, recur_depth=3, V=2),
    "depth0": dict(first_nbins=8, recur_depth=0),
    "depth1_r3": dict(first_nbins=8, recur_depth=1, recur_nbins=3, seed=2),
    "batch3": dict(B=3, first_nbins=8, recur_depth=2, per_sample_limbs=True, seed=3),
    "batch4": dict(B=4, tree="star", first_nbins=5, grid_size=1200.0, tolerance=160.0, recur_depth=2, per_sample_limbs=True, seed=4),
    "small_maps": dict(H=8, W=8, first_nbins=8, recur_depth=2, seed=5),
    "nonsquare": dict(H=64, W=48, first_nbins=8, recur_depth=2, seed=6),
    "distorted": dict(first_nbins=8, recur_depth=2, distortion=True, seed=7),
    "zero_ties": dict(first_nbins=8, grid_size=6000.0, recur_depth=2, seed=8),      # bins outside every view, most limbs out of reach
    "nan": dict(tree="chain", first_nbins=5, grid_size=1200.0, tolerance=160.0, recur_depth=2, nan=True, seed=9),
}
GOLDEN_CASES = {     # what make_golden_rpsm.py runs through the reference
    "g4": dict(first_nbins=4, grid_size=600.0, recur_depth=3, seed=11),
    "g8": dict(first_nbins=8, recur_depth=10, seed=12),
    "g8_dist": dict(first_nbins=8, recur_depth=4, distortion=True, V=3, seed=13),
    "g16": dict(B=2, first_nbins=16, recur_depth=10, seed=14),
}
ATTEMPTS = 8


def attempt_inputs(name, attempt):
    kw = dict(CASES[name] if name in CASES else GOLDEN_CASES[name])
    kw["seed"] = kw.get("seed", 0) + 1000 * attempt
    return inputs(**kw)


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of the case and their restatement, from the first seed on which conditions (a) and (b) hold; read-only"""
    for attempt in range(ATTEMPTS):
        inp = attempt_inputs(name, attempt)
        if boundary_distance(inp) < MARGIN_A:
            continue
        ref = solve(inp)
        if conditions(inp, ref):
            for a in list(inp.values()) + list(ref.values()):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            return inp, ref, attempt
    raise AssertionError("%s: no seed in %d attempts meets conditions (a) and (b)" % (name, ATTEMPTS))


def golden():
    g = np.load(os.path.join(GOLD, "rpsm.npz"))
    return {k: g[k] for k in g.files}


def ulps(a, b):
    """|a - b| in units of the float32 spacing at b"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)
